"""Distribution checks of the vector path's counter-based randomness (Philox4x32-10 keyed by the
run seed): the learner's with-replacement replay sampling (robot.py:98-115 draws a permutation
prefix; the vector path draws uniform indices), the target-policy smoothing noise
(robot.py:338-339: clamp(0.2 z, +-0.5)) and the exploration noise (robot.py:614-620:
noise_scale * max_action * z). The N = 1 drop-in consumes numpy's stream instead and is pinned bit
for bit elsewhere; here the statistics are the contract. Each test reads the kernels' outputs with
the networks zeroed so the outputs expose the draws directly. Thresholds: p > 1e-4 for the
chi-square / KS tests (fixed seeds, so the outcome is deterministic), moments within 5 standard
errors. The second half pins the same three streams value for value against the oracle's
restatements (oracle.sample_indices / smoothing_noise / learner_counters), directly and through
a whole td3_update: a wrong counter word, a dropped seed_hi, an index drawn over the ring's
capacity or two batches sharing a counter all pass the statistics."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import stats

from gpu_support import nav  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _zero_net(d_in, d_out, hidden=64, nh=2):
    from nav.mlp import DeviceMLP
    net = DeviceMLP(d_in, d_out, hidden, nh, DEV)
    net.params.zero_()
    net.pack()
    return net


def test_replay_sampling_uniform_with_replacement(nav):
    """train_critic's and train_actor's Philox batches: every index of the ring equally likely,
    the two batches of one epoch and of consecutive epochs different streams."""
    from nav import config as K
    from nav._lib import stream_handle
    from nav.td3 import TD3
    from nav.vec_env import ReplayRing
    size, B = 1000, 32768
    cfg = K.TD3Config(batch_size=B, num_epochs=1, net=K.NetConfig(hidden=64, n_hidden=2))
    td3 = TD3(cfg, device=DEV, seed=12345)
    ring = ReplayRing(4096, DEV)
    ring.rows[:size, 0] = torch.arange(size, dtype=torch.float32, device=DEV)  # s0 = own index
    ring.size = size
    s = stream_handle()
    draws = []
    for counter in range(2):
        td3.update_counter = counter
        td3._critic_rows(ring, None, None, s)
        torch.cuda.synchronize()
        draws.append(td3.batch[:, 0].long().cpu())
        td3._actor_rows(ring, None, s)
        torch.cuda.synchronize()
        draws.append(td3.batch2[:, 0].long().cpu())
    for d in draws:
        assert d.min() >= 0 and d.max() < size
        counts = torch.bincount(d, minlength=size).numpy()
        assert stats.chisquare(counts).pvalue > 1e-4
        # with replacement: duplicates at the birthday rate of B draws over `size` indices
        assert len(np.unique(d.numpy())) == (counts > 0).sum()
    for i in range(len(draws)):
        for j in range(i + 1, len(draws)):
            assert (draws[i] == draws[j]).float().mean() < 0.01  # independent streams
    # the same (seed, counter) reproduces its batch exactly
    td3.update_counter = 0
    td3._critic_rows(ring, None, None, s)
    torch.cuda.synchronize()
    assert torch.equal(td3.batch[:, 0].long().cpu(), draws[0])


def test_target_smoothing_noise_distribution(nav):
    """Target policy smoothing (robot.py:338-339) through nav_mlp_forward's OUT_TARGET with a zero
    target actor: out = clamp(clamp(0.2 z, +-0.5), +-5) with z ~ N(0, 1) per (row, output)."""
    from nav.mlp import forward
    net = _zero_net(2, 2)
    M = 65536
    x = torch.randn(M, 2, device=DEV)
    out = torch.zeros(M, 2, device=DEV)
    forward([net], x, 2, 0, [out], 2, 0, M, out_mode=1, eps=None, policy_noise=0.2,
            noise_clip=0.5, max_action=5.0, seed=(7, 0), counter=3)
    v = out.cpu().double().numpy()
    assert np.abs(v).max() <= 0.5
    z = v / 0.2
    clipped = np.abs(z) >= 2.5 - 1e-6
    p_clip = 2 * stats.norm.sf(2.5)
    n = z.size
    assert abs(clipped.mean() - p_clip) < 5 * np.sqrt(p_clip * (1 - p_clip) / n)
    # the unclipped part against N(0, 1) truncated to |z| < 2.5
    core = z[~clipped]
    tn = stats.truncnorm(-2.5, 2.5)
    assert stats.kstest(core, tn.cdf).pvalue > 1e-4
    assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 5 / np.sqrt(M)
    # another counter gives another draw
    out2 = torch.zeros_like(out)
    forward([net], x, 2, 0, [out2], 2, 0, M, out_mode=1, eps=None, seed=(7, 0), counter=4)
    assert (out2 == out).float().mean() < 0.05


def test_exploration_noise_distribution(nav):
    """Exploration noise of get_next_action_training (robot.py:614-620) through nav_act with a
    zero actor and state = goal: action = clip(noise_scale * max_action * z, +-5), z ~ N(0, 1)
    per (env, coordinate), a fresh draw per step."""
    from nav._lib import lib, params_struct, ptr, stream_handle
    net = _zero_net(2, 2)
    n = 65536
    p = params_struct(seed_lo=99, seed_hi=0)
    state = (torch.rand(n, 2, dtype=torch.float64, device=DEV) * 90 + 5).contiguous()
    goal = state.clone()
    scale = torch.full((n,), 0.1, dtype=torch.float64, device=DEV)  # sigma = 0.1 * 5 = 0.5
    acts = []
    for step in (0, 1):
        a = torch.zeros(n, 2, dtype=torch.float64, device=DEV)
        rc = lib().nav_act(C.byref(p), C.byref(net.desc()), n, ptr(state), ptr(goal), ptr(scale),
                           None, step, 0, ptr(a), None, stream_handle())
        assert rc == 0
        torch.cuda.synchronize()
        acts.append(a.cpu().numpy() / 0.5)
    for z in acts:
        assert stats.kstest(z.ravel(), "norm").pvalue > 1e-4
        assert abs(z.mean()) < 5 / np.sqrt(z.size)
        assert abs(z.std() - 1) < 5 * np.sqrt(0.5 / z.size)
        assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 5 / np.sqrt(n)
    assert abs(np.corrcoef(acts[0].ravel(), acts[1].ravel())[0, 1]) < 5 / np.sqrt(2 * n)
    # testing mode (robot.py:572-595): no noise at all
    a = torch.zeros(n, 2, dtype=torch.float64, device=DEV)
    lib().nav_act(C.byref(p), C.byref(net.desc()), n, ptr(state), ptr(goal), ptr(scale), None, 0,
                  1, ptr(a), None, stream_handle())
    torch.cuda.synchronize()
    assert torch.count_nonzero(a).item() == 0


# ---- the same three streams value for value against the oracle's restatements ----
SEED = (0x5A17 << 32) | 424242  # seed_hi != 0: a dropped high word shows


def test_replay_sampling_values_vs_oracle(nav, orc):
    """train_critic's and train_actor's Philox batches at update_counter 5 and 6 equal
    oracle.sample_indices with the counters of oracle.learner_counters, index for index. The ring
    holds 4 096 rows filled to 1 000 (an index drawn over the capacity would leave the fill), its
    s0 column the row's own index."""
    from nav import config as K
    from nav._lib import stream_handle
    from nav.td3 import TD3
    from nav.vec_env import ReplayRing
    size, B = 1000, 16421
    cfg = K.TD3Config(batch_size=B, num_epochs=1, net=K.NetConfig(hidden=64, n_hidden=2))
    td3 = TD3(cfg, device=DEV, seed=SEED)
    ring = ReplayRing(4096, DEV)
    ring.rows[:, 0] = torch.arange(4096, dtype=torch.float32, device=DEV)
    ring.size = size
    p = orc.default_params(SEED)
    s = stream_handle()
    for counter in (5, 6):
        ctr = orc.learner_counters(counter)
        td3.update_counter = counter
        td3._critic_rows(ring, None, None, s)
        td3._actor_rows(ring, None, s)
        torch.cuda.synchronize()
        got_c = td3.batch[:, 0].long().cpu().numpy()
        got_a = td3.batch2[:, 0].long().cpu().numpy()
        assert np.array_equal(got_c, orc.sample_indices(p, B, size, ctr["critic_sample"])), counter
        assert np.array_equal(got_a, orc.sample_indices(p, B, size, ctr["actor_sample"])), counter
        assert not np.array_equal(got_c, got_a)


def test_target_smoothing_noise_values_vs_oracle(nav, orc):
    """OUT_TARGET through a zeroed target actor equals clamp(0.2 * oracle.smoothing_noise, +-0.5)
    within 1e-6 absolute for every (row, output) of 65 536 rows (the device's Box-Muller differs
    from libm's by a few f64 ulp, which the f32 rounding can turn into one f32 ulp of |z| < 8:
    under 1e-7 after the 0.2).
    Measured on MI355X: max |diff| 0 (all 131 072 values bit-equal), 1.24 % clamped."""
    from nav.mlp import forward
    net = _zero_net(2, 2)
    M, counter = 65536, 3
    x = torch.randn(M, 2, device=DEV)
    out = torch.full((M, 2), float("nan"), device=DEV)
    forward([net], x, 2, 0, [out], 2, 0, M, out_mode=1, eps=None, policy_noise=0.2,
            noise_clip=0.5, max_action=5.0, seed=(SEED & 0xFFFFFFFF, SEED >> 32), counter=counter)
    p = orc.default_params(SEED)
    eps = orc.smoothing_noise(p, M, counter)
    want = np.clip(eps * np.float32(0.2), np.float32(-0.5), np.float32(0.5))
    d = np.abs(out.cpu().numpy().astype(np.float64) - want.astype(np.float64))
    print(f"max |diff| {d.max():.2e}, exact {np.mean(d == 0):.4f}, clamped "
          f"{np.mean(np.abs(want) == 0.5):.4f}")
    assert d.max() <= 1e-6
    assert 0.005 < np.mean(np.abs(want) == 0.5) < 0.03  # 2 sf(2.5) = 1.2 %: both sides of the clamp




def _relu_decisions_within_band(net, x, bits, tag):
    """The kernel's ReLU bits of `net` (an oracle MLP holding the same weights) on input rows x
    equal torch's f32 (z > 0) wherever |z| is outside the f32 summation-order band K 1.2e-7
    (|h| |W|^T + |b|) of test_backward_and_weight_grads_vs_autograd; returns the number of
    decisions that differ inside it."""
    h, n = x, 0
    for l, (W, b) in enumerate(net.params[:-1]):
        z = torch.nn.functional.linear(h, W, b)
        band = W.shape[1] * 1.2e-7 * (h.abs() @ W.abs().t() + b.abs())
        differ = (z > 0) != bits[l]
        assert not (differ & (z.abs() > band)).any(), (tag, l)
        n += int(differ.sum())
        h = torch.relu(z)
    return n


def test_td3_update_on_philox_path_vs_oracle(nav, orc):
    """TD3.td3_update with idx_fn = eps_fn = None (the product path: batches and smoothing noise
    drawn in the kernels) against TD3Oracle fed oracle.sample_indices / oracle.smoothing_noise:
    2x256 nets, B = 16 421 (64-row blocks, ragged last block), a 50 000-row ring filled to 40 000
    with the unfilled rows NaN (a read outside the fill poisons the loss), seed_hi != 0,
    update_counter from 5, 2 epochs (critic, actor + Polyak, critic). Bounds of
    test_td3_update_at_bench_config_vs_oracle: losses rtol 1e-4, every parameter within 2e-7.

    Three learners on the same ring: (u) td3_update with nothing injected; (i) td3_update with
    the restated draws injected as idx_fn / eps_fn; (s) train_critic / train_actor called epoch
    by epoch with nothing injected, so that each epoch's ReLU bit images can be read. (s) equals
    (u) bit for bit, (i) equals (u) within the parameter bound, and the oracle is compared with
    (s). The oracle takes the kernels' ReLU decisions (TD3Oracle's `bits`, as
    test_learner_gradients_at_bench_config_vs_oracle does), checked here against the oracle's own
    f32 pre-activations outside the rounding band: with its own decisions one row of 16 421
    whose pre-activation is within rounding of 0 (|z| = 9.5e-7) branches the other way in unit 2
    of critic 1's layer 1, a unit alive on 130 rows of the batch, which turns the sign of an
    8e-5 weight-gradient entry of that unit and with it Adam's first step: 11 entries of that
    one weight row end 2.2e-7 .. 1.04e-5 from the plain oracle, every other parameter within
    3e-8 (measured on MI355X; the figure is printed).
    Measured on MI355X: max |diff| vs the oracle actor 7.5e-9, critic 1 1.5e-8, critic 2 3.0e-8,
    targets <= 1.2e-10; (i) bit-identical to (u); losses equal to 5e-8 relative."""
    from mlp_ref import relu_bits
    from pop_support import make_learner, replay_rows
    from nav.vec_env import ReplayRing
    from oracle.td3_oracle import TD3Oracle, make_mlp_params
    B, hidden, nh, epochs, cap, fill, c0 = 16421, 256, 2, 2, 50000, 40000, 5
    sizes = lambda di, do: [di] + [hidden] * nh + [do]  # noqa: E731
    params = (make_mlp_params(181, sizes(2, 2)), make_mlp_params(182, sizes(4, 1)),
              make_mlp_params(183, sizes(4, 1)))
    rows = replay_rows(fill, 29)
    rep = ReplayRing(cap, DEV)
    rep.rows.fill_(float("nan"))
    rep.rows[:fill] = torch.tensor(rows, device=DEV)
    rep.size = fill
    p = orc.default_params(SEED)
    draws_i, draws_n = [], []
    for epoch in range(epochs):
        ctr = orc.learner_counters(c0 + epoch)
        draws_i.append(orc.sample_indices(p, B, fill, ctr["critic_sample"]))
        draws_n.append(orc.smoothing_noise(p, B, ctr["smoothing"]))
        if epoch % 2 == 0:
            draws_i.append(orc.sample_indices(p, B, fill, ctr["actor_sample"]))

    def learner():
        td3 = make_learner(B, hidden, nh, params)
        td3.seed = SEED
        td3.update_counter = c0
        return td3

    def feeds():
        it = {"s": 0, "n": 0}

        def sample():
            x = draws_i[it["s"]]; it["s"] += 1
            return x

        def nz():
            x = draws_n[it["n"]]; it["n"] += 1
            return x
        return it, sample, nz

    def batch_of(i):
        r = rows[i]
        return r[:, 0:2], r[:, 2:4], r[:, 4], r[:, 5:7], r[:, 7] > 0.5

    # (u) the product path, nothing injected
    lu = learner()
    lu.td3_update(rep, num_epochs=epochs, track_losses=True)
    torch.cuda.synchronize()
    assert lu.update_counter == c0 + epochs
    assert np.isfinite(lu.critic_losses).all() and np.isfinite(lu.actor_losses).all()
    # (i) the restated draws injected
    li = learner()
    it, sample, nz = feeds()
    li.td3_update(rep, num_epochs=epochs,
                  idx_fn=lambda: torch.tensor(sample(), dtype=torch.int64, device=DEV),
                  eps_fn=lambda: torch.tensor(nz(), device=DEV))
    torch.cuda.synchronize()
    assert it == {"s": len(draws_i), "n": len(draws_n)}
    # (s) epoch by epoch, the oracles in step: `ora` on the kernels' ReLU decisions, `plain` on
    # its own
    ls = learner()
    ora, plain = TD3Oracle(*params), TD3Oracle(*params)
    it, sample, nz = feeds()
    hp = ls.critic_network_1.hp
    closs, aloss, in_band = [], [], 0
    for epoch in range(epochs):
        ls.train_critic(rep)
        torch.cuda.synchronize()
        i, eps = sample(), nz()
        assert np.array_equal(ls.batch.cpu().numpy(), rows[i]), epoch  # the rows it trained on
        bits = {"c1": relu_bits(ls.mask1, nh, hp, hidden, B),
                "c2": relu_bits(ls.mask2, nh, hp, hidden, B)}
        x = torch.tensor(rows[i][:, 0:4])
        in_band += _relu_decisions_within_band(ora.critic1, x, bits["c1"], ("c1", epoch))
        in_band += _relu_decisions_within_band(ora.critic2, x, bits["c2"], ("c2", epoch))
        closs.append(ora.train_critic(batch_of(i), eps, bits=bits))
        plain.train_critic(batch_of(i), eps)
        if epoch % 2 == 0:
            ls.train_actor(rep, soft_update=True)
            torch.cuda.synchronize()
            i = sample()
            assert np.array_equal(ls.batch2.cpu().numpy()[:, [0, 1, 4, 5, 6, 7]],
                                  rows[i][:, [0, 1, 4, 5, 6, 7]]), epoch
            bits = {"actor": relu_bits(ls.mask_a, nh, hp, hidden, B),
                    "c1": relu_bits(ls.mask1, nh, hp, hidden, B)}
            s0 = torch.tensor(rows[i][:, 0:2])
            in_band += _relu_decisions_within_band(ora.actor, s0, bits["actor"], ("actor", epoch))
            aloss.append(ora.train_actor(rows[i][:, 0:2], bits=bits))
            ora.soft_update()
            plain.train_actor(rows[i][:, 0:2])
            plain.soft_update()
        ls.update_counter += 1
    assert in_band <= 16, in_band  # decisions inside the band are rare events, not a pattern
    print(f"ReLU decisions that differ from torch f32 inside the rounding band: {in_band}")
    print("critic losses", lu.critic_losses, np.mean(closs, 1), "actor", lu.actor_losses, aloss)
    np.testing.assert_allclose(lu.critic_losses, np.mean(closs, 1), rtol=1e-4)
    np.testing.assert_allclose(lu.actor_losses, aloss, rtol=1e-4)
    flat = lambda layers: torch.cat([t.reshape(-1) for wb in layers for t in wb])  # noqa: E731
    for name, onet in ora.networks().items():
        got = flat(lu.networks()[name].export())
        assert torch.isfinite(got).all(), name
        assert torch.equal(lu.networks()[name].params, ls.networks()[name].params), name
        d_i = float((got - flat(li.networks()[name].export())).abs().max())
        d_o = float((got - flat(onet.params)).abs().max())
        d_p = (got - flat(plain.networks()[name].params)).abs()
        print(f"{name}: max |diff| vs oracle {d_o:.3e}, vs the injected learner {d_i:.3e}; vs the "
              f"oracle on its own ReLU decisions {float(d_p.max()):.3e} "
              f"({int((d_p > 2e-7).sum())} entries over 2e-7)")
        assert d_i <= 2e-7, name
        assert d_o <= 2e-7, name
