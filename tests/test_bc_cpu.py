"""Learning from demonstrations, the parts that need no GPU: the new entry points' host-side
argument checks (no kernel is launched), the numpy restatement of nav_demo_transitions against a
hand-written demonstration, and the conditions the GPU tests of tests/test_gpu_bc.py rely on,
established here on the CPU (the ReLU band cap for the fp32 chain of the BC cases, and that 200
Adam steps of pure BC lower the BC loss)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bc_ref as BR
import mlp_ref as R


@pytest.fixture(scope="module")
def navlib():
    from nav import _lib
    return _lib.lib()


def _mlp(d_in, d_out):
    from nav._lib import NavMlp
    return NavMlp(d_in, d_out, 64, 64, 2, 16, 16)


def _actor_rows_bc(navlib, critic=True, B=64, b_demo=16, bc_weight=0.5, bc_part=16, actor=True):
    """The raw status of nav_td3_actor_rows_bc on dummy pointers (never followed: an accepted
    call would launch, so every case here has to be refused)."""
    from nav._lib import NavReplay
    a, c, rd = _mlp(2, 2), _mlp(4, 1), NavReplay(16, 1000)
    p = C.c_void_p
    return navlib.raw.nav_td3_actor_rows_bc(
        C.byref(a) if actor else None, C.byref(c) if critic else None, C.byref(rd), 500, B, None,
        1, 2, 3, b_demo, 1.0, bc_weight, p(16), p(16), p(16), p(bc_part) if bc_part else None,
        None, 0, None, 0, p(16), p(16), p(16), None)


def test_actor_rows_bc_rejects_inconsistent_arguments(navlib):
    from nav._lib import NAV_EINVAL
    assert _actor_rows_bc(navlib, b_demo=65) == NAV_EINVAL            # B_demo > B
    assert _actor_rows_bc(navlib, b_demo=-1) == NAV_EINVAL
    assert _actor_rows_bc(navlib, b_demo=0, bc_weight=0.5) == NAV_EINVAL  # a weight on no rows
    assert _actor_rows_bc(navlib, bc_part=None) == NAV_EINVAL
    assert _actor_rows_bc(navlib, actor=False) == NAV_EINVAL
    assert _actor_rows_bc(navlib, critic=False, b_demo=65) == NAV_EINVAL
    assert _actor_rows_bc(navlib, B=0, b_demo=0, bc_weight=0.0) == NAV_EINVAL
    # the plain entry point still needs its critic
    from nav._lib import NavReplay
    a, rd, p = _mlp(2, 2), NavReplay(16, 1000), C.c_void_p
    assert navlib.raw.nav_td3_actor_rows(C.byref(a), None, C.byref(rd), 500, 64, None, 1, 2, 3,
                                         p(16), p(16), p(16), None, 0, None, 0, p(16), p(16),
                                         p(16), None) == NAV_EINVAL


def test_mix_idx_rejects_inconsistent_arguments(navlib):
    from nav._lib import NAV_EINVAL
    mix = navlib.raw.nav_td3_mix_idx
    p = C.c_void_p
    assert mix(500, 100, 101, 500, 37, 1, 2, 3, p(16), p(16), None) == NAV_EINVAL  # B_demo > B
    assert mix(500, 100, 7, 500, 0, 1, 2, 3, p(16), p(16), None) == NAV_EINVAL     # no demo rows
    assert mix(500, 100, -1, 500, 37, 1, 2, 3, p(16), p(16), None) == NAV_EINVAL
    assert mix(0, 100, 7, 500, 37, 1, 2, 3, p(16), p(16), None) == NAV_EINVAL
    assert mix(500, 0, 0, 500, 37, 1, 2, 3, p(16), p(16), None) == NAV_EINVAL
    assert mix(500, 100, 7, -1, 37, 1, 2, 3, p(16), p(16), None) == NAV_EINVAL
    assert mix(500, 100, 7, 500, 37, 1, 2, 3, None, None, None) == 0  # nothing to write


def test_demo_transitions_rejects_inconsistent_arguments(navlib):
    from nav._lib import NAV_EINVAL, params_struct
    f = navlib.raw.nav_demo_transitions
    p, v = params_struct(), C.c_void_p
    assert f(C.byref(p), 2, 5, v(16), v(16), v(16), 2, v(16), None) == NAV_EINVAL   # frame
    assert f(C.byref(p), 2, 5, v(16), v(16), v(16), -1, v(16), None) == NAV_EINVAL
    assert f(C.byref(p), 0, 5, v(16), v(16), v(16), 0, v(16), None) == NAV_EINVAL
    assert f(C.byref(p), 2, 1, v(16), v(16), v(16), 0, v(16), None) == NAV_EINVAL   # no transition
    assert f(None, 2, 5, v(16), v(16), v(16), 0, v(16), None) == NAV_EINVAL
    for hole in range(4):
        args = [v(16)] * 4
        args[hole] = None
        assert f(C.byref(p), 2, 5, args[0], args[1], args[2], 0, args[3], None) == NAV_EINVAL


def test_transitions_restatement_against_a_hand_written_demonstration():
    """Four transitions towards the goal (10, 20): the second s' lies 0.099 outside the goal
    threshold (distance sqrt(26)), the third exactly on it (distance 5 counts as reached:
    robot.py:744's >=), the fourth at the goal; the first action is beyond +-5 (CEM's raw action,
    kept in frame 0, clamped in frame 1)."""
    from nav.demo_replay import transitions_ref
    st = np.array([[[30, 20], [22, 20], [15, 21], [13, 24], [10, 20]]], np.float32)
    ac = np.array([[[-8, 0.5], [-5, 1], [-2, 3], [-3, -4], [9, 9]]], np.float32)
    g = np.array([[10.0, 20.0]])
    r0 = transitions_ref(st, ac, g, 0)
    want0 = np.array([
        [30, 20, -8, 0.5, -12.0, 22, 20, 0],
        [22, 20, -5, 1, -np.sqrt(26.0), 15, 21, 0],
        [15, 21, -2, 3, 50.0, 13, 24, 0],          # |(3, 4)| = 5 >= -threshold: goal_reward
        [13, 24, -3, -4, 50.0, 10, 20, 1]], np.float64).astype(np.float32)
    assert np.array_equal(r0, want0)
    r1 = transitions_ref(st, ac, g, 1)
    want1 = np.array([
        [20, 0, -5 - 20, 0.5 - 0, -12.0, 12, 0, 0],   # clamp(-8) = -5
        [12, 0, -5 - 12, 1 - 0, -np.sqrt(26.0), 5, 1, 0],
        [5, 1, -2 - 5, 3 - 1, 50.0, 3, 4, 0],
        [3, 4, -3 - 3, -4 - 4, 50.0, 0, 0, 1]], np.float64).astype(np.float32)
    assert np.array_equal(r1, want1)
    # a second demonstration shifts the rows by T - 1 and uses its own goal
    st2 = np.concatenate([st, st + 1], 0)
    ac2 = np.concatenate([ac, ac], 0)
    r = transitions_ref(st2, ac2, np.array([[10.0, 20.0], [11.0, 21.0]]), 0)
    assert r.shape == (8, 8) and np.array_equal(r[4:, 4], r0[:, 4])
    assert np.array_equal(r[4:, 0:2], r0[:, 0:2] + 1)


def test_goal_term_restatement_is_the_ticks_norm(orc):
    """transitions_ref's -norm against the oracle's norm2 (sqrt(fma(y, y, x * x)), the tick's)
    on values whose squares do not round alike with and without the fused step."""
    from nav.demo_replay import _neg_norm
    g = np.random.RandomState(3)
    for _ in range(2000):
        x, y = (g.standard_normal(2) * 10 ** g.uniform(-3, 2)).tolist()
        assert _neg_norm(x, y) == -orc.lib().orc_norm2(x, y)


def test_replay_ring_tail_shares_the_allocation():
    """ReplayRing(tail=n): one [capacity + n][8] allocation, `rows` its first capacity rows (what
    desc(), advance() and the ticks see), `tail` the rest; without a tail, and with a `rows=`
    slice of a population's tensor, the ring is what it was."""
    from nav.vec_env import ReplayRing
    ring = ReplayRing(8, "cpu", tail=3)
    assert ring.storage.shape == (11, 8) and ring.rows.shape == (8, 8) and ring.tail.shape == (3, 8)
    assert ring.rows.data_ptr() == ring.storage.data_ptr() == ring.desc().rows
    assert ring.tail.data_ptr() == ring.storage.data_ptr() + 8 * 8 * 4
    assert ring.rows.is_contiguous() and ring.tail.is_contiguous() and ring.desc().capacity == 8
    assert ring.advance(5) == 0 and ring.advance(5) == 5
    assert (len(ring), ring.position) == (8, 2)
    plain = ReplayRing(8, "cpu")
    assert plain.tail.shape == (0, 8) and plain.storage.shape == (8, 8)
    pool = torch.zeros(2, 8, 8)
    member = ReplayRing(8, "cpu", rows=pool[1])
    assert member.rows.data_ptr() == pool[1].data_ptr() and member.tail.shape[0] == 0
    with pytest.raises(AssertionError):
        ReplayRing(8, "cpu", rows=pool[1], tail=3)


# ---- the conditions the GPU tests rely on ----
BC_SHAPES = [(24, 1), (90, 2), (200, 3), (256, 2)]
BC_CASES = [(h, nh, B, bd) for h, nh in BC_SHAPES for B in (33, 100) for bd in (0, 7, B)]
BC_CASES.append((150, 2, 16421, 4100))


@pytest.mark.parametrize("hidden,nh,B,b_demo", BC_CASES,
                         ids=["-".join(map(str, c)) for c in BC_CASES])
def test_fp32_chain_of_the_bc_cases_stays_inside_the_band_cap(hidden, nh, B, b_demo):
    """relu_band / assert_band_cap is a condition of the fp64 comparison on the GPU: the fp32
    chain's own ReLU decisions on the BC cases (the ring plus the demonstration tail) stay
    inside it, for the actor and for the critic on (s, pi(s))."""
    case = BR.bc_case(hidden, nh, B, b_demo)
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
    R.assert_band_cap(inside + i2, entries + e2)


def test_bc_reference_is_the_autograd_gradient():
    """actor_epoch_bc (the reference of the GPU tests) against torch autograd of the loss as the
    header states it, with and without the critic."""
    case = BR.bc_case(24, 2, 33, 7)
    rows = case["rows"][case["idx_a"]]
    la, lc = case["layers"]["actor"], case["layers"]["cr0"]
    for critic in (lc, None):
        params = [(W.double().requires_grad_(), b.double().requires_grad_()) for W, b in la]
        s = rows[:, :2].double()
        a = R.torch_mlp(params, s)
        bc = ((a[:7] - rows[:7, 2:4].double()) ** 2).sum() / 7
        loss = R.f32c(0.5) * bc
        if critic is not None:
            q = R.torch_mlp([(W.double(), b.double()) for W, b in critic], torch.cat([s, a], 1))
            loss = loss - q.mean()
        loss.backward()
        bits_a = BR.forward_bits(la, s)
        bits_c = None if critic is None else BR.forward_bits(lc, torch.cat([s, a.detach()], 1))
        ref = BR.actor_epoch_bc(la, critic, rows, bits_a, bits_c, 7, 1.0, 0.5)
        assert torch.allclose(ref["bc"] / 7, bc.detach().reshape(1), rtol=1e-12)
        for (gW, gb), (W, b) in zip(ref["grads"], params):
            # f32(2 * 0.5 / 7) and f32(-1 / 33) are the launch's coefficients: 6e-8 relative
            assert torch.allclose(gW, W.grad, rtol=1e-6, atol=1e-7 * float(W.grad.abs().max()))
            assert torch.allclose(gb, b.grad, rtol=1e-6, atol=1e-7 * float(b.grad.abs().max()))


def test_pure_bc_adam_steps_lower_the_bc_loss_in_torch():
    """The torch restatement of VecTrainer.pretrain_bc(epochs=200, lr=1e-3) at the trainer test's
    shape (hidden 64, 2 layers, batch 128): 200 Adam steps on mean_b sum_j (pi_j(s_b) - a_{b,j})^2
    over batches drawn with replacement from acting-frame demonstration rows lower the loss over
    all rows. The rows are of the kind nav_demo_transitions produces: paths of 200 steps towards
    a goal, residual = clamp(a) - (s - g)."""
    g = torch.Generator().manual_seed(11)
    n_demo, T = 6, 200
    start = (torch.rand(n_demo, 1, 2, generator=g) - 0.5) * 120
    t = torch.linspace(1, 0, T).view(1, T, 1)
    s = start * t + torch.randn(n_demo, T, 2, generator=g)          # s - g along the path
    a = (torch.randn(n_demo, T, 2, generator=g) * 3).clamp(-5, 5)   # the clipped action
    rows_s = s[:, :-1].reshape(-1, 2)
    rows_a = (a[:, :-1] - s[:, :-1]).reshape(-1, 2)
    from oracle.td3_oracle import make_mlp_params
    p = make_mlp_params(5, [2, 64, 64, 2])
    params = [(torch.tensor(W).requires_grad_(), torch.tensor(b).requires_grad_()) for W, b in p]
    opt = torch.optim.Adam([t_ for wb in params for t_ in wb], lr=1e-3)

    def loss_all():
        with torch.no_grad():
            return float(((R.torch_mlp(params, rows_s) - rows_a) ** 2).sum(1).mean())

    before = loss_all()
    for _ in range(200):
        idx = torch.randint(0, rows_s.shape[0], (128,), generator=g)
        opt.zero_grad()
        ((R.torch_mlp(params, rows_s[idx]) - rows_a[idx]) ** 2).sum(1).mean().backward()
        opt.step()
    after = loss_all()
    print(f"bc loss {before:.4f} -> {after:.4f}")
    assert after < before
