"""The Q-filter of the behaviour-cloning term on the GPU: nav_td3_actor_rows_bcq bit for bit
against nav_td3_actor_rows_bc and nav_mlp_forward where it does what they do, against the fp64
restatement of tests/bcq_ref.py where it does not, and the trainer and the population with
bc_q_filter.

Cases (tests/bcq_ref.py CASES; all but the last launch 32-row blocks, B <= 16384; the last one
64-row blocks): every launch of a case is made once and shared by the tests (module cache).
Bars: tests/mlp_ref.py's, as tests/test_gpu_bc.py uses them (row quantities 2e-6 of scale,
cross-row sums 1e-5, each at least 8 x the fp32 chain's own error). The conditions on the inputs
(kept / dropped / undecided shares) are established on the CPU in tests/test_bcq_cpu.py and
asserted again here from the same fp64 numbers."""
import ctypes as C
import functools

import pytest
import torch

import bcq_ref as Q
import launches as LN
import mlp_ref as R
from gpu_support import equal_nan as _equal_nan, ids as _ids, nav  # noqa: F401
from launches import nan as _nan
from pop_support import equal_tree as _equal_tree, member_state, same as _same, snapshot

pytestmark = pytest.mark.gpu
DEV = R.DEV
NAN = float("nan")
W_BC = 0.5   # bc_weight of the cases (q_weight 1)


@functools.lru_cache(maxsize=None)
def _setup(hidden, nh, B, b_demo):
    case = Q.bcq_case(hidden, nh, B, b_demo)
    return (case, *LN.device_epoch(case))


def _launch(key, b_demo, bc_weight, form, grads=False):
    """nav_td3_actor_rows_bcq (form "bcq") or nav_td3_actor_rows_bc ("bc") of case `key` into
    NaN-prefilled buffers (keep_part prefilled with -1), q_weight 1; grads: then nav_mlp_wgrad and
    nav_grad_reduce into the actor's flat gradient `g`."""
    _, nets, dev = _setup(*key)
    o = LN.actor_rows(nets, dev, key[2], form=form, fill=NAN, b_demo=b_demo, q_weight=1.0,
                     bc_weight=bc_weight)
    if grads:
        o["g"], = LN.flat_grads([nets["actor"]], o, fill=NAN)
    torch.cuda.synchronize()
    return o


@functools.lru_cache(maxsize=None)
def _run(key):
    """The case's Q-filtered launch (with gradients), the kernel's own decisions keep_b = q_demo[b]
    > q[b], and the fp64 / fp32 restatements with the kernel's ReLU bits and decisions injected,
    plus the fp64 restatement that decides by itself."""
    hidden, nh, B, b_demo = key
    case, nets, _ = _setup(*key)
    o = _launch(key, b_demo, W_BC, "bcq", grads=True)
    rows_a = case["rows"][case["idx_a"]]
    assert torch.equal(o["batch"].cpu(), rows_a)
    keep = (o["q_demo"][:b_demo] > o["q"][:b_demo]).cpu()
    hp = nets["actor"].hp
    la, lc = case["layers"]["actor"], case["layers"]["cr0"]
    bits_a = R.relu_bits(o["ma"], nh, hp, hidden, B)
    bits_c = R.relu_bits(o["mc"], nh, hp, hidden, B)
    args = (la, lc, rows_a, b_demo, 1.0, W_BC)
    ref = Q.bcq_epoch(*args, keep=keep, bits_a=bits_a, bits_c=bits_c)
    f32 = Q.bcq_epoch(*args, keep=keep, bits_a=bits_a, bits_c=bits_c, dtype=torch.float32)
    own = Q.bcq_epoch(*args)
    return dict(o=o, keep=keep, ref=ref, f32=f32, own=own, rows=rows_a, tm=32 if B <= 16384 else 64)


SHAPES = sorted({c[:3] for c in Q.CASES})


@pytest.mark.parametrize("hidden,nh,B", SHAPES, ids=_ids(SHAPES))
def test_without_demonstration_rows_it_is_the_bc_form(nav, hidden, nh, B):
    """4. B_demo = 0 (bc_weight 0): every output equals nav_td3_actor_rows_bc's bit for bit
    (rows the launch leaves alone stay NaN in both), keep_part is all 0, q_demo untouched."""
    key = next(c for c in Q.CASES if c[:3] == (hidden, nh, B))
    a = _launch(key, 0, 0.0, "bcq", grads=True)
    b = _launch(key, 0, 0.0, "bc", grads=True)
    for k in ("batch", "q", "da", "dz", "acts", "ma", "mc", "es", "part", "g"):
        assert _equal_nan(a[k].float(), b[k].float()), k
    assert bool((a["part"] == 0).all()) and bool((a["keep_part"] == 0).all())
    assert bool(a["q_demo"].isnan().all())


@pytest.mark.parametrize("key", Q.CASES, ids=_ids(Q.CASES))
def test_q_demo_is_the_critics_forward(nav, key):
    """5. q_demo[:B_demo] equals nav_mlp_forward of critic 1 on the returned batch (ld_in 8,
    in_col 0; all B rows, so the 32-row tiles are the launch's) bit for bit, rows >= B_demo are
    not written, and it lies within the row bar of the fp64 restatement. Scale: max |Q1(s_b, a_b)|
    over the batch's rows (the forward runs on whole blocks; a single demonstration row's own
    value is no scale for an fp32 chain's error)."""
    from nav._lib import lib, ptr, stream_handle
    hidden, nh, B, b_demo = key
    r = _run(key)
    o, case = r["o"], _setup(*key)[0]
    cr = _setup(*key)[1]["cr0"]
    out = _nan(B)
    assert lib().nav_mlp_forward(C.byref(cr.desc()), 1, B, ptr(o["batch"]), 8, 0,
                                 (C.c_void_p * 1)(out.data_ptr()), 1, 0, 0, None, 0.0, 0.0, 0.0,
                                 0, 0, 0, None, 0, None, stream_handle()) == 0
    torch.cuda.synchronize()
    assert torch.equal(o["q_demo"][:b_demo], out[:b_demo])
    assert bool(o["q_demo"][b_demo:].isnan().all())
    lc = case["layers"]["cr0"]
    x = r["rows"][:, :4]
    q64, q32 = R.mlp_forward(lc, x)[0][:, 0], R.mlp_forward(lc, x, torch.float32)[0][:, 0]
    assert torch.equal(q64[:b_demo], r["own"]["q_demo"])
    scale = float(q64.abs().max())
    err = float((o["q_demo"][:b_demo].cpu().double() - q64[:b_demo]).abs().max()) / scale
    e32 = float((q32[:b_demo].double() - q64[:b_demo]).abs().max()) / scale
    print(f"q_demo: err {err:.2e} e32 {e32:.2e} bar {R.bar('q_demo', e32):.1e}")
    assert err <= R.bar("q_demo", e32)


@pytest.mark.parametrize("key", Q.CASES, ids=_ids(Q.CASES))
def test_decision_and_da_against_the_bc_form(nav, key):
    """6. With keep_b := q_demo[b] > q[b] from the kernel's own outputs: row b < B_demo of da
    equals nav_td3_actor_rows_bc's with bc_weight = w where keep_b and with bc_weight = 0 where
    not, rows >= B_demo equal both; q, batch and the critic's mask words equal the BC form's;
    keep_part is the per-block count of keep; bc_part's sum is within 1e-6 relative of the fp64
    sum over the kept rows."""
    hidden, nh, B, b_demo = key
    r = _run(key)
    o, keep, tm = r["o"], r["keep"], r["tm"]
    on, off = _launch(key, b_demo, W_BC, "bc"), _launch(key, b_demo, 0.0, "bc")
    kd = keep.to(DEV)
    da, d_on, d_off = o["da"], on["da"], off["da"]
    assert bool(torch.isfinite(da).all())
    assert torch.equal(da[:b_demo][kd], d_on[:b_demo][kd])
    assert torch.equal(da[:b_demo][~kd], d_off[:b_demo][~kd])
    assert torch.equal(da[b_demo:], d_on[b_demo:]) and torch.equal(da[b_demo:], d_off[b_demo:])
    if 0 < int(keep.sum()):  # the weight does enter on kept rows
        assert not torch.equal(d_on[:b_demo][kd], d_off[:b_demo][kd])
    for k in ("q", "batch", "mc", "ma"):
        assert torch.equal(o[k], on[k]), k
    assert o["nblk"] == (B + tm - 1) // tm
    full = torch.zeros(o["nblk"] * tm, dtype=torch.int32)
    full[:b_demo] = keep.int()
    assert torch.equal(o["keep_part"].cpu(), full.view(-1, tm).sum(1).int())
    part = o["part"].cpu()
    assert bool(torch.isfinite(part).all())
    assert bool((part[(b_demo + tm - 1) // tm:] == 0).all())
    got, want = float(part.double().sum()), float(r["ref"]["bc"])
    print(f"bc_part sum {got!r} fp64 {want!r} rel {abs(got - want) / max(want, 1e-300):.2e}")
    assert abs(got - want) <= 1e-6 * want


@pytest.mark.parametrize("key", Q.CASES, ids=_ids(Q.CASES))
def test_filter_is_exercised_and_agrees_with_fp64(nav, key):
    """7. On every decided row (fp64 margin |q_demo - q_pi| at least 1e-5 of max |q|) the kernel's
    keep equals fp64's. Conditions on the inputs, from fp64 alone: undecided rows at most 2 % of
    the demonstration rows, kept and dropped each at least 5 % (not for a single row)."""
    b_demo = key[3]
    r = _run(key)
    own = r["own"]
    kept, dropped, undecided, und = Q.filter_shares(own)
    print(f"kept {kept:.3f} dropped {dropped:.3f} undecided {undecided:.4f} "
          f"kernel kept {float(r['keep'].sum()) / b_demo:.3f}")
    assert undecided <= 0.02
    if b_demo > 1:
        assert kept >= 0.05 and dropped >= 0.05
    assert torch.equal(r["keep"][~und], own["keep"][~und])


@pytest.mark.parametrize("key", Q.CASES, ids=_ids(Q.CASES))
def test_gradients_vs_fp64(nav, key):
    """8. q, da, the filtered BC sum and the actor's flat gradient (nav_mlp_wgrad + reduce) tensor
    by tensor against the fp64 restatement given the kernel's keep mask and ReLU bits, at the bars
    tests/test_gpu_bc.py holds the same quantities to."""
    hidden, nh, B, b_demo = key
    r = _run(key)
    o, case, nets = r["o"], *_setup(*key)[:2]
    hp = nets["actor"].hp
    ref, f32 = r["ref"], r["f32"]
    la, lc = case["layers"]["actor"], case["layers"]["cr0"]
    # the condition of the injected bits: they are the fp64 signs outside the rounding band
    bits_a = R.relu_bits(o["ma"], nh, hp, hidden, B)
    bits_c = R.relu_bits(o["mc"], nh, hp, hidden, B)
    s = r["rows"][:, :2]
    _, zs_a, _ = R.mlp_forward(la, s)
    inside, entries = R.relu_band(la, s, zs_a, bits_a)
    a64 = R.mlp_forward(la, s)[0]
    x_c = torch.cat([s.double(), a64], 1)
    _, zs_c, _ = R.mlp_forward(lc, x_c)
    a32 = R.mlp_forward(la, s, torch.float32)[0]
    bar_a = R.bar("a", R.rel_err(a32, a64)) * float(a64.abs().max())
    extra = torch.full((1, 2), bar_a, dtype=torch.float64) @ lc[0][0][:, 2:4].double().abs().t()
    i2, e2 = R.relu_band(lc, x_c, zs_c, bits_c, extra0=extra)
    R.assert_band_cap(inside + i2, entries + e2)
    d = dict(da=o["da"].cpu(), loss_bc=o["part"].cpu().double().sum().reshape(1), q=o["q"].cpu())
    if 0 < b_demo < B:
        d.update(da_demo=d["da"][:b_demo], da_rest=d["da"][b_demo:])
    d.update(R.flat_grad_tensors(o["g"].cpu(), 2, 2, hidden, hp, nh))
    over = R.ParityLog().judge(hp, nh, "actor_rows_bcq",
                               R.compare(d, Q.bcq_quantities(ref), Q.bcq_quantities(f32)))
    assert not over, over


# ---- 9. the trainer and the population ----
TRAINER = dict(n_envs=256, envs_per_group=128, hidden=64, n_hidden=2, batch=256,
               updates_per_step=2)
ON = dict(demo_fraction=0.25, bc_weight=1.0)


def _learner_state(tr):
    return snapshot(tr, "moments", ring="storage")


def _steps(tr, n=3):
    for _ in range(n):
        tr.step()
    torch.cuda.synchronize()
    return tr


def test_trainer_with_the_filter(nav, tmp_path):
    """Three steps with demo_fraction 0.25, bc_weight 1 and bc_q_filter: it runs through the
    Q-filtered launch, the kept share lies in [0, 1] and is the workspace's count, a checkpoint
    saved and loaded continues bit for bit; bc_q_filter=False is a trainer built without the
    argument, bit for bit."""
    from nav.trainer import VecTrainer
    tr = _steps(VecTrainer(device=DEV, bc_q_filter=True, **ON, **TRAINER))
    t = tr.td3
    assert t.cfg.bc_q_filter and t._last_b_demo == 64 == t.b_demo()
    kept = t.bc_kept_fraction()
    print(f"bc_kept_fraction {kept:.4f} bc_loss {t.bc_loss_value():.4f}")
    assert 0.0 <= kept <= 1.0 and kept == int(t.keep_part.sum()) / 64
    assert int(t.keep_part.min()) >= 0 and bool((t.keep_part[2:] == 0).all())
    want = (t.q_demo[:64] > t.q1[:64])
    assert int(want.sum()) == int(t.keep_part.sum())
    assert bool(torch.isfinite(t.actor_network.params).all()) and t.bc_loss_value() >= 0
    path = str(tmp_path / "bcq.pt")
    tr.save(path)
    c = VecTrainer.load(path, device=DEV)
    assert c.td3.cfg.bc_q_filter is True
    tr.step()
    c.step()
    torch.cuda.synchronize()
    assert _same(_learner_state(tr), _learner_state(c))
    assert c.td3.bc_kept_fraction() == tr.td3.bc_kept_fraction()
    off = _steps(VecTrainer(device=DEV, bc_q_filter=False, **ON, **TRAINER))
    plain = _steps(VecTrainer(device=DEV, **ON, **TRAINER))
    assert _same(_learner_state(off), _learner_state(plain))
    assert off.td3.bc_kept_fraction() == 0.0 and "bc_q_filter" not in off.state_dict()["meta"]
    # a checkpoint from before the argument loads with the filter off
    assert VecTrainer.from_state_dict(plain.state_dict(), device=DEV).td3.cfg.bc_q_filter is False


POP = dict(hidden=64, n_hidden=2, batch=128, updates_per_step=2, seed=1234, envs_per_group=128)


def _member_state(tr, m):
    """Member m's ring with its tail and its learner (the envs of a mixed population's member are
    not compared with a lone trainer's here)."""
    s = member_state(tr, m, tail=True)
    return {**s["replay"], "td3": s["td3"]}


def test_population_members_learner_takes_the_key(nav):
    """P = 2 with learner="members" and bc_q_filter on member 0 alone: member 0 ends as a lone
    VecTrainer with the key (ring with its tail, every parameter and moment), member 1 as member
    1 of the population where nobody has the key (the plain BC member)."""
    from nav.population import PopulationTrainer
    from nav.trainer import VecTrainer

    def pop(members):
        return _steps(PopulationTrainer(members, envs_per_member=256, device=DEV,
                                        learner="members", **POP))
    mixed = pop([dict(ON, bc_q_filter=True), dict(ON)])
    plain = pop([dict(ON), dict(ON)])
    lone = _steps(VecTrainer(n_envs=256, device=DEV, bc_q_filter=True, **ON, **POP))
    assert mixed.td3[0].cfg.bc_q_filter and not mixed.td3[1].cfg.bc_q_filter
    assert 0.0 <= mixed.td3[0].bc_kept_fraction() <= 1.0 and mixed.td3[1].bc_kept_fraction() == 0.0
    _equal_tree(_member_state(mixed, 1), _member_state(plain, 1), "member 1")
    want = {"rows": lone.replay.storage, "position": lone.replay.position,
            "size": lone.replay.size, "td3": lone.td3.state_dict()}
    _equal_tree(_member_state(mixed, 0), want, "member 0")
    assert mixed.td3[0].bc_kept_fraction() == lone.td3.bc_kept_fraction()
