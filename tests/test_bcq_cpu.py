"""The Q-filter of the behaviour-cloning term, the parts that need no GPU: the restatement of
tests/bcq_ref.py pinned by a hand-worked case and by its two identities (every row kept = the
unfiltered BC loss of tests/bc_ref.py, no row kept = the plain actor loss), the conditions on the
inputs the GPU tests of tests/test_gpu_bcq.py rely on, nav_td3_actor_rows_bcq's host-side
argument checks (no kernel is launched) and the ValueErrors of the config, the trainer and the
population."""
import ctypes as C

import pytest
import torch

import bc_ref as BR
import bcq_ref as Q
import mlp_ref as R


# ---- 1. the restatement ----
def _t(*rows):
    return torch.tensor(rows, dtype=torch.float32)


def test_restatement_on_a_hand_worked_case():
    """One hidden unit, three rows, B_demo = 2, q_weight 1, bc_weight 0.5.
    Actor: h = relu(s_0), pi = (h, 2 h). Critic: Q(s, a) = relu(a_0 + a_1).
    row 0: s = (1, 0), a = (2, 3): pi = (1, 2), Q_pi = 3 < Q_demo = 5: kept, (pi - a) = (-1, -1)
    row 1: s = (2, 0), a = (1, 1): pi = (2, 4), Q_pi = 6 > Q_demo = 2: dropped
    row 2: s = (3, 0), a = (100, 100): pi = (3, 6), Q_pi = 9; Q_demo would pass, not a demo row.
    With cq = f32(-1/3) and the BC coefficient f32(2 * 0.5 / 2) = 0.5:
    dL/da = cq * (1, 1) on every row, + 0.5 * (-1, -1) on row 0; the BC sum is 2."""
    actor = [(_t([1, 0]), _t(0).reshape(1)), (_t([1], [2]), _t(0, 0).reshape(2))]
    critic = [(_t([0, 0, 1, 1]), _t(0).reshape(1)), (_t([1]), _t(0).reshape(1))]
    batch = _t([1, 0, 2, 3, 0, 0, 0, 0], [2, 0, 1, 1, 0, 0, 0, 0], [3, 0, 100, 100, 0, 0, 0, 0])
    e = Q.bcq_epoch(actor, critic, batch, 2, 1.0, 0.5)
    cq = R.f32c(-1.0 / 3)
    d = torch.float64
    assert torch.equal(e["q"], torch.tensor([3, 6, 9], dtype=d))
    assert torch.equal(e["q_demo"], torch.tensor([5, 2], dtype=d))
    assert e["keep"].tolist() == [True, False]
    assert torch.equal(e["bc"], torch.tensor([2], dtype=d))
    want_da = torch.tensor([[cq - 0.5] * 2, [cq] * 2, [cq] * 2], dtype=d)
    assert torch.allclose(e["da"], want_da, rtol=0, atol=1e-15)
    (dW0, db0), (dWo, dbo) = e["grads"]
    # dWo_j = sum_b da_bj h_b with h = (1, 2, 3); dh_b = da_b0 + 2 da_b1 = 3 da_b0
    close = lambda got, want: torch.allclose(  # noqa: E731
        got, torch.tensor(want, dtype=d).reshape(got.shape), rtol=0, atol=1e-14)
    assert close(dWo, [6 * cq - 0.5, 6 * cq - 0.5]) and close(dbo, [3 * cq - 0.5] * 2)
    assert close(dW0, [18 * cq - 1.5, 0.0]) and close(db0, [9 * cq - 1.5])
    # the critic's gradient is that of -mean Q(s, pi(s)) alone: the filter carries none
    (cW0, cb0), (cWo, cbo) = e["grads_c"]
    assert close(cWo, [18 * cq]) and close(cbo, [3 * cq]) and close(cb0, [3 * cq])
    assert close(cW0, [6 * cq, 0.0, 6 * cq, 12 * cq])
    # the other decision on row 1 is the mask's to make: both rows kept adds its term
    e2 = Q.bcq_epoch(actor, critic, batch, 2, 1.0, 0.5, keep=torch.tensor([True, True]))
    assert torch.equal(e2["bc"], torch.tensor([2 + 1 + 9], dtype=d))
    assert close(e2["da"][1], [cq + 0.5 * 1, cq + 0.5 * 3])
    # strict: a tie is dropped (row 0's demonstrated action moved to Q_demo = 3 = Q_pi)
    tie = batch.clone()
    tie[0, 2:4] = _t(1, 2)
    assert Q.bcq_epoch(actor, critic, tie, 2, 1.0, 0.5)["keep"].tolist() == [False, False]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_restatement_identities(dtype):
    """Mask all ones: da, the BC sum and the gradients of bc_ref.actor_epoch_bc (the unfiltered
    form's reference). Mask all zeros: those of mlp_ref.actor_epoch with the BC term absent."""
    h, nh, B, bd = 24, 2, 33, 7
    case = Q.bcq_case(h, nh, B, bd, seed=1)
    rows = case["rows"][case["idx_a"]]
    la, lc = case["layers"]["actor"], case["layers"]["cr0"]
    s = rows[:, :2]
    bits_a = BR.forward_bits(la, s)
    a64 = R.mlp_forward(la, s)[0]
    bits_c = BR.forward_bits(lc, torch.cat([s.double(), a64], 1))
    tol = dict(rtol=1e-11, atol=1e-13) if dtype == torch.float64 else dict(rtol=2e-4, atol=1e-6)

    def same(e, ref, tol=tol):
        assert torch.allclose(e["da"], ref["da"], **tol)
        assert torch.allclose(e["q"], ref["q"], **tol)
        for (gW, gb), (rW, rb) in zip(e["grads"], ref["grads"]):
            assert torch.allclose(gW, rW, **tol) and torch.allclose(gb, rb, **tol)

    ones = Q.bcq_epoch(la, lc, rows, bd, 0.75, 0.5, keep=torch.ones(bd, dtype=torch.bool),
                       bits_a=bits_a, bits_c=bits_c, dtype=dtype)
    ref = BR.actor_epoch_bc(la, lc, rows, bits_a, bits_c, bd, 0.75, 0.5, dtype=dtype)
    same(ones, ref)
    assert torch.allclose(ones["bc"], ref["bc"], **tol)
    zeros = Q.bcq_epoch(la, lc, rows, bd, 1.0, 0.5, keep=torch.zeros(bd, dtype=torch.bool),
                        bits_a=bits_a, bits_c=bits_c, dtype=dtype)
    # (actor_epoch seeds the critic with -1 / B itself, the launch with its f32 value: 3e-8)
    same(zeros, R.actor_epoch(la, lc, rows, bits_a, bits_c, dtype=dtype),
         dict(rtol=max(tol["rtol"], 1e-7), atol=tol["atol"]))
    assert float(zeros["bc"]) == 0.0


@pytest.mark.parametrize("hidden,nh,B,b_demo", Q.CASES,
                         ids=["-".join(map(str, c)) for c in Q.CASES])
def test_cases_meet_the_input_conditions(hidden, nh, B, b_demo):
    """Conditions on the inputs of the GPU tests, from the fp64 restatement alone: undecided
    rows (margin below 1e-5 of max |q|) at most 2 % of the demonstration rows, kept and dropped
    each at least 5 % of them (a single demonstration row: decided, either way)."""
    case = Q.bcq_case(hidden, nh, B, b_demo)
    rows = case["rows"][case["idx_a"]]
    assert float(rows[:, :2].min()) >= 0 and float(rows[:, :2].max()) <= 100
    assert float(rows[:, 2:4].abs().max()) <= 5
    ref = Q.bcq_epoch(case["layers"]["actor"], case["layers"]["cr0"], rows, b_demo, 1.0, 0.5)
    kept, dropped, undecided, _ = Q.filter_shares(ref)
    print(f"kept {kept:.3f} dropped {dropped:.3f} undecided {undecided:.4f}")
    assert undecided <= 0.02
    if b_demo > 1:
        assert kept >= 0.05 and dropped >= 0.05


@pytest.mark.parametrize("hidden,nh,B,b_demo", Q.CASES,
                         ids=["-".join(map(str, c)) for c in Q.CASES])
def test_fp32_chain_of_the_cases_stays_inside_the_band_cap(hidden, nh, B, b_demo):
    """relu_band / assert_band_cap is a condition of the GPU gradient comparison (the kernel's
    ReLU bits are injected into fp64): the fp32 chain's own decisions on these cases stay inside
    it, for the actor and for the critic on (s, pi(s)), as tests/test_bc_cpu.py shows for the BC
    cases."""
    case = Q.bcq_case(hidden, nh, B, b_demo)
    rows = case["rows"][case["idx_a"]]
    la, lc = case["layers"]["actor"], case["layers"]["cr0"]
    s = rows[:, :2]
    a64, zs_a, _ = R.mlp_forward(la, s)
    a32, zs_a32, _ = R.mlp_forward(la, s, torch.float32)
    inside, entries = R.relu_band(la, s, zs_a, [z > 0 for z in zs_a32])
    x = torch.cat([s.double(), a64], 1)
    _, zs_c, _ = R.mlp_forward(lc, x)
    _, zs_c32, _ = R.mlp_forward(lc, torch.cat([s, a32], 1), torch.float32)
    bar_a = R.bar("a", R.rel_err(a32, a64)) * float(a64.abs().max())
    extra = torch.full((1, 2), bar_a, dtype=torch.float64) @ lc[0][0][:, 2:4].double().abs().t()
    i2, e2 = R.relu_band(lc, x, zs_c, [z > 0 for z in zs_c32], extra0=extra)
    print(f"inside the band {inside + i2} of {entries + e2}")
    R.assert_band_cap(inside + i2, entries + e2)


# ---- 2. host refusals ----
@pytest.fixture(scope="module")
def navlib():
    from nav import _lib
    return _lib.lib()


def _mlp(d_in, d_out):
    from nav._lib import NavMlp
    return NavMlp(d_in, d_out, 64, 64, 2, 16, 16)


def _bcq(navlib, critic=True, B=64, b_demo=16, bc_weight=0.5, bc_part=True, actor=True, q=True,
         keep_part=True, q_demo=True, masks_critic=True):
    """The raw status of nav_td3_actor_rows_bcq on dummy pointers (never followed: an accepted
    call would launch, so every case here has to be refused)."""
    from nav._lib import NavReplay
    a, c, rd = _mlp(2, 2), _mlp(4, 1), NavReplay(16, 1000)
    p = lambda on: C.c_void_p(16) if on else None  # noqa: E731
    return navlib.raw.nav_td3_actor_rows_bcq(
        C.byref(a) if actor else None, C.byref(c) if critic else None, C.byref(rd), 500, B, None,
        1, 2, 3, b_demo, 1.0, bc_weight, p(True), p(q), p(True), p(bc_part), p(q_demo),
        p(keep_part), None, 0, None, 0, p(True), p(masks_critic), p(True), None)


def test_actor_rows_bcq_rejects_inconsistent_arguments(navlib):
    from nav._lib import NAV_EINVAL
    assert _bcq(navlib, critic=False) == NAV_EINVAL        # the filter needs a critic
    assert _bcq(navlib, keep_part=False) == NAV_EINVAL
    assert _bcq(navlib, q=False) == NAV_EINVAL
    # what the BC form refuses
    assert _bcq(navlib, b_demo=65) == NAV_EINVAL           # B_demo > B
    assert _bcq(navlib, b_demo=-1) == NAV_EINVAL
    assert _bcq(navlib, b_demo=0, bc_weight=0.5) == NAV_EINVAL  # a weight on no rows
    assert _bcq(navlib, bc_part=False) == NAV_EINVAL
    assert _bcq(navlib, actor=False) == NAV_EINVAL
    assert _bcq(navlib, B=0, b_demo=0, bc_weight=0.0) == NAV_EINVAL
    assert _bcq(navlib, masks_critic=False) == NAV_EINVAL
    assert _bcq(navlib, critic=False, q_demo=False, b_demo=65) == NAV_EINVAL


# ---- the config, the trainer and the population ----
def test_config_refuses_the_filter_without_a_bc_term():
    from nav import config as K
    assert K.TD3Config().bc_q_filter is False
    assert K.TD3Config(batch_size=100, demo_fraction=0.25, bc_weight=1.0,
                       bc_q_filter=True).b_demo() == 25
    with pytest.raises(ValueError, match="bc_q_filter"):
        K.TD3Config(batch_size=100, bc_q_filter=True).b_demo()
    with pytest.raises(ValueError, match="bc_q_filter"):  # demonstration rows, no weight
        K.TD3Config(batch_size=100, demo_fraction=0.25, bc_q_filter=True).b_demo()
    with pytest.raises(ValueError):  # 0.004 * 100 rounds to no row
        K.TD3Config(batch_size=100, demo_fraction=0.004, bc_weight=1.0, bc_q_filter=True).b_demo()
    # the unfiltered refusals are what they were
    with pytest.raises(ValueError, match="bc_weight needs"):
        K.TD3Config(batch_size=100, bc_weight=1.0).b_demo()
    assert K.TD3Config(batch_size=100).b_demo() == 0


@pytest.mark.parametrize("kw", [dict(), dict(demo_fraction=0.25), dict(bc_weight=1.0),
                                dict(demo_fraction=0.001, bc_weight=1.0)],
                         ids=["alone", "no_weight", "no_rows", "rounds_to_0"])
def test_trainer_refuses_before_it_builds(kw):
    from nav.trainer import VecTrainer
    with pytest.raises(ValueError, match="bc_q_filter|bc_weight needs"):
        VecTrainer(n_envs=256, hidden=64, batch=128, bc_q_filter=True, **kw)


def test_population_refuses_the_batched_learner_and_a_bare_filter():
    from nav.population import PBT_EXPLORE_KEYS, TD3_KEYS, PopulationTrainer
    assert "bc_q_filter" in TD3_KEYS and "bc_q_filter" not in PBT_EXPLORE_KEYS
    member = {"demo_fraction": 0.25, "bc_weight": 1.0, "bc_q_filter": True}
    with pytest.raises(ValueError, match=r"bc_q_filter.*member 1"):
        PopulationTrainer([{}, member], envs_per_member=64, hidden=64, batch=64,
                          envs_per_group=64, learner="batched")
    with pytest.raises(ValueError, match=r"member 0.*bc_q_filter"):
        PopulationTrainer([{"bc_q_filter": True}, {}], envs_per_member=64, hidden=64, batch=64,
                          envs_per_group=64)
