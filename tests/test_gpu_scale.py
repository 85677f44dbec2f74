"""The MLP kernels across operand magnitudes: exact rescaling by powers of two.

Every hidden x hidden product is an fp32 GEMM emulated on the fp16 matrix cores, and its
correctness rests on power-of-two scales computed at run time (the A scale per 32-row tile of
gemm_cols_whole / gemm_cols_step, the per-column exponents of k_pack_img's images and of the Wt =
Wo . W product image, gemm_bits' unscale, the operand scales of k_wgrad, k_wgrad_fact and
k_wgrad_gen, pow2_exp_to's clamp). The property tested here pins all of it at once: multiply the
inputs by 2^a, layer l's weights by 2^k_l, its bias by 2^(a + k_0 + .. + k_l) and the incoming
gradient by 2^g, and every f32 chain yields the base run's values times a known power of two, bit
for bit, while nothing leaves the normal f32 range (tests/test_scale_cpu.py establishes that for
the fp32 torch chain at every case used here). The kernels must do the same: the scaled operands
land in the same [2^13, 2^14) window, so the fp16 planes and the accumulators are the same bits,
and ldexpf is exact. One mis-tracked exponent, an early clamp or a stray absolute constant breaks
bit equality on thousands of entries; no tolerance is involved (mlp_ref.assert_shifted).

(3) the unfused chain and the packed images under the shift sets S1 .. S3, (4) the fused TD3
launches, the BC form, the population forms and the acting launches under joint shifts (critics of
total K, reward column 2^K, actors of total 0), (5) the ends of the range R1 .. R5, where clamps
and caps may legitimately bind, against the fp64 chain at the project's unchanged bars; with
NAV_SCALE_PARITY=<file> the worst figures of (5) are written there at the end of the module (the
source of profiles/scale_range_parity.txt)."""
import ctypes as C
import os

import pytest
import torch

import bc_ref as BR
import launches as LN
import mlp_ref as R
import pop_support as T
from gpu_support import equal_nan, nav  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = R.DEV
LOG = R.ParityLog()
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _parity_log():
    """At the end of the module: the worst figures of (5), where NAV_SCALE_PARITY names a file."""
    yield
    path = os.environ.get("NAV_SCALE_PARITY")
    if path:
        LOG.write(path)


def _ids(cases):
    return [str(c).replace(" ", "") for c in cases]


# ---- (3) the unfused chain under S1 .. S3 ----
_runs = {}


def chain_run(shape, M, name=None):
    """unfused_chain_run (5 splits, NaN-prefilled gradient buffers) of the base case (name None)
    or under shift set `name`; computed once per case."""
    key = (shape, M, name)
    if key not in _runs:
        shift = None if name is None else R.shift_set(name, shape[3])
        _runs[key] = R.unfused_chain_run(*shape, M, nan_fill=True, shift=shift)
    return _runs[key]


def run_quantities(run, shape):
    """A run's quantities by name at logical sizes; the padded columns of the saved rows and the
    padded rows, columns and slots of the flat gradient must be exactly 0."""
    d_in, d_out, hidden, nh = shape
    assert bool((run["acts"][:, :, hidden:] == 0).all())
    assert bool((run["dz"][:, :, hidden:] == 0).all())
    q = dict(out=run["out"], dx=run["dx"])
    for l in range(nh):
        q[f"h{l}"], q[f"dz{l}"] = run["acts"][l][:, :hidden], run["dz"][l][:, :hidden]
    q.update(R.flat_grad_tensors(run["grad"], d_in, d_out, hidden, run["net"].hp, nh))
    return q


@pytest.mark.parametrize("name", list(R.SHIFT_SETS))
@pytest.mark.parametrize("shape,M", R.SCALE_CHAIN_CASES, ids=_ids(R.SCALE_CHAIN_CASES))
def test_unfused_chain_is_shift_equivariant(nav, shape, M, name):
    """nav_mlp_forward -> nav_mlp_backward -> nav_mlp_wgrad (5 splits) -> nav_grad_reduce of the
    rescaled case against the base run: out, every h_l, dz_l, dx and every tensor of the reduced
    flat gradient equal the base's times their power of two bit for bit, the ReLU bit images are
    equal, the padding is exactly 0 in both runs."""
    base, run = chain_run(shape, M), chain_run(shape, M, name)
    q0, q1 = run_quantities(base, shape), run_quantities(run, shape)
    assert torch.equal(run["masks"], base["masks"])
    exp = R.expected_shifts(*R.shift_set(name, shape[3]))
    assert exp.keys() == q0.keys()
    for n in q0:
        assert bool((q0[n] != 0).any()), n
        R.assert_shifted(q1[n], q0[n], exp[n], f"{shape} M {M} {name} {n}")


IMAGE_SHAPES = [s for s in R.SCALE_SHAPES if s[3] >= 2]


@pytest.mark.parametrize("name", list(R.SHIFT_SETS))
@pytest.mark.parametrize("shape", IMAGE_SHAPES, ids=_ids(IMAGE_SHAPES))
def test_packed_images_carry_the_layer_shift(nav, shape, name):
    """After DeviceMLP.load of the rescaled layers both fp16 planes of every forward and backward
    image equal the base net's bit for bit, and every logical column's exponent is the base's
    minus the layer's shift (the top backward image of a d_out = 1 net, Wt = Wo . W: minus
    k_{nh-1} + k_nh); the padded columns' exponents stay 0. Both nets' images are also the exact
    split of their own weights (mlp_ref._assert_images_exact)."""
    d_in, d_out, hidden, nh = shape
    _, ks, _ = R.shift_set(name, nh)
    n0, n1 = chain_run(shape, 97)["net"], chain_run(shape, 97, name)["net"]
    hp = n0.hp
    R._assert_images_exact(n0, "base")  # (the absolute exponents and planes, at both magnitudes)
    R._assert_images_exact(n1, name)
    p0, p1 = n0.packed.detach().cpu(), n1.packed.detach().cpu()
    img = hp * hp + hp
    for L in range(1, nh):
        for which, off in (("fwd", (L - 1) * 2 * img), ("bwd", (L - 1) * 2 * img + img)):
            k = ks[L]
            if which == "bwd" and d_out == 1 and L == nh - 1:
                k += ks[nh]
            (P0, e0), (P1, e1) = R._fp16_image(p0, off, hp), R._fp16_image(p1, off, hp)
            assert bool((P0 != 0).any())
            assert torch.equal(P1, P0), (L, which)
            assert torch.equal(e1[:hidden], e0[:hidden] - k), (L, which, k)
            assert bool((e1[hidden:] == 0).all()) and bool((e0[hidden:] == 0).all())


# ---- (4) the fused launches under joint shifts ----
def _assert_batch(got, base, K):
    """A sampled batch under the joint shift: the reward column times 2^K, the rest equal."""
    keep = [0, 1, 2, 3, 5, 6, 7]
    assert torch.equal(got[:, keep], base[:, keep])
    R.assert_shifted(got[:, 4], base[:, 4], K, "batch reward")


def _critic_launches(hidden, nh, B, K):
    """nav_td3_critic_rows -> nav_mlp_wgrad (nav_mlp_wgrad_splits) -> nav_grad_reduce of
    epoch_case(hidden, nh, B, K) as test_fused_critic_epoch_vs_fp64 issues them: CPU tensors."""
    nets, dev = LN.device_epoch(R.epoch_case(hidden, nh, B, K))
    cr = [nets["cr0"], nets["cr1"]]
    o = LN.critic_rows(nets, dev, B, fill=NAN, split=0)
    grads = LN.flat_grads(cr, o, fill=NAN)
    torch.cuda.synchronize()
    q = dict(batch=o["batch"].cpu(), masks=[m.cpu() for m in o["masks"]])
    for k in range(2):
        q[f"c{k}_dq"], q[f"c{k}_loss"] = o["dq"][k].cpu(), o["lp"][k].cpu()
        q.update({f"c{k}_{n}": t for n, t in R.flat_grad_tensors(grads[k].cpu(), 4, 1, hidden,
                                                                 cr[0].hp, nh).items()})
    return q


def _actor_quantities(o, g, hidden, hp, nh):
    q = dict(batch=o["batch"].cpu(), masks=[o["ma"].cpu(), o["mc"].cpu()], a_q=o["q"].cpu(),
             a_da=o["da"].cpu())
    q.update({f"a_{n}": t for n, t in R.flat_grad_tensors(g.cpu(), 2, 2, hidden, hp, nh).items()})
    return q


def _actor_launches(hidden, nh, B, K):
    """nav_td3_actor_rows -> nav_mlp_wgrad -> nav_grad_reduce as test_fused_actor_epoch_vs_fp64
    issues them: CPU tensors."""
    nets, dev = LN.device_epoch(R.epoch_case(hidden, nh, B, K))
    o = LN.actor_rows(nets, dev, B, form="plain", fill=NAN)
    g, = LN.flat_grads([nets["actor"]], o, fill=NAN)
    torch.cuda.synchronize()
    return _actor_quantities(o, g, hidden, nets["actor"].hp, nh)


_epochs = {}


def epoch_launches(kind, hidden, nh, B, K=None):
    key = (kind, hidden, nh, B, K)
    if key not in _epochs:
        _epochs[key] = (_critic_launches if kind == "critic" else _actor_launches)(hidden, nh, B, K)
    return _epochs[key]


def _assert_epoch(got, base, exp, K, tag):
    _assert_batch(got["batch"], base["batch"], K)
    for m1, m0 in zip(got["masks"], base["masks"]):
        assert torch.equal(m1, m0)
    names = [n for n in base if n not in ("batch", "masks")]
    assert set(names) <= exp.keys()
    for n in names:
        assert bool((base[n] != 0).any()), n
        R.assert_shifted(got[n], base[n], exp[n], f"{tag} {n}")


def critic_shifts(nh, K):
    """The exponents of the critic launches' outputs: dq K, the blocks' loss parts 2 K, the
    gradients those of a chain with the critic's layer shifts and incoming gradient 2^K."""
    ec = R.expected_shifts(0, R.joint_shifts(nh, K)[1], K)
    s = {}
    for k in range(2):
        s.update({f"c{k}_dq": K, f"c{k}_loss": 2 * K})
        s.update({f"c{k}_{n}": ec[n] for n in R.grad_names(nh)})
    return s


def actor_shifts(nh, K):
    """q and da carry K, the actor's gradients K plus its own layers' shifts."""
    ea = R.expected_shifts(0, R.joint_shifts(nh, K)[0], K)
    s = dict(a_q=K, a_da=K)
    s.update({f"a_{n}": ea[n] for n in R.grad_names(nh)})
    return s


@pytest.mark.parametrize("K", R.SCALE_KS)
@pytest.mark.parametrize("hidden,nh,B", R.SCALE_EPOCH_CASES, ids=_ids(R.SCALE_EPOCH_CASES))
def test_fused_critic_epoch_is_shift_equivariant(nav, hidden, nh, B, K):
    """nav_td3_critic_rows -> nav_mlp_wgrad -> nav_grad_reduce with every critic's layers shifted
    by a total of K, the reward column by 2^K and both actors by shifts of total 0: the sampled
    rows but for the reward, and the ReLU bits, are unchanged; dq carries K, every block's loss
    part 2 K, both critics' gradients their chain's shifts, bit for bit."""
    _assert_epoch(epoch_launches("critic", hidden, nh, B, K), epoch_launches("critic", hidden, nh, B),
                  critic_shifts(nh, K), K, f"critic_rows {hidden} x {nh} B {B} K {K}")


@pytest.mark.parametrize("K", R.SCALE_KS)
@pytest.mark.parametrize("hidden,nh,B", R.SCALE_EPOCH_CASES, ids=_ids(R.SCALE_EPOCH_CASES))
def test_fused_actor_epoch_is_shift_equivariant(nav, hidden, nh, B, K):
    """nav_td3_actor_rows -> nav_mlp_wgrad -> nav_grad_reduce under the same joint shifts: the
    actions keep their magnitude (both ReLU bit images unchanged), q and da carry K, the actor's
    gradients K plus its own layers' shifts, bit for bit."""
    _assert_epoch(epoch_launches("actor", hidden, nh, B, K), epoch_launches("actor", hidden, nh, B),
                  actor_shifts(nh, K), K, f"actor_rows {hidden} x {nh} B {B} K {K}")


def test_actor_rows_bc_is_shift_equivariant(nav):
    """nav_td3_actor_rows_bc at (150, 2), B = 100, 7 demonstration rows, q_weight 1 and the BC
    weight 0.5 * 2^K, so that both terms of da carry K: q, da and the gradients shift, the
    blocks' BC sums (of (pi - a)^2, unweighted) and the sampled rows do not."""
    hidden, nh, B, bd = 150, 2, 100, 7
    runs = {}
    for K in (None,) + R.SCALE_KS:
        nets, dev = LN.device_epoch(BR.bc_case(hidden, nh, B, bd, K=K))
        o = LN.actor_rows(nets, dev, B, form="bc", fill=NAN, b_demo=bd, q_weight=1.0,
                          bc_weight=0.5 * 2.0 ** (K or 0))
        g, = LN.flat_grads([nets["actor"]], o, fill=NAN)
        torch.cuda.synchronize()
        runs[K] = dict(_actor_quantities(o, g, hidden, nets["actor"].hp, nh), part=o["part"].cpu())
    for K in R.SCALE_KS:
        exp = dict(actor_shifts(nh, K), part=0)
        _assert_epoch(runs[K], runs[None], exp, K, f"actor_rows_bc K {K}")


def _pop_run(Ks):
    """Two members (pop_support.make_td3's, hidden 64 x 2, B = 100) through
    nav_td3_actor_rows_pop and nav_td3_critic_rows_pop, each followed by its group's
    nav_mlp_wgrad_pop and nav_grad_reduce_adam_pop (for the reduced gradients; the actor phase
    first, so that neither row launch reads a network Adam has stepped). Ks[m]: member m's joint
    shift, or None. Returns per member the outputs by name."""
    from nav._lib import lib, ptr, stream_handle
    from nav.population import PopulationLearner
    hidden, nh, B, P = 64, 2, 100, 2
    rings = [T.make_ring(m) for m in range(P)]
    td3 = [T.make_td3(m, hidden, nh, B, 1) for m in range(P)]
    for t, ring, K in zip(td3, rings, Ks):
        if K is None:
            continue
        ka, kc = R.joint_shifts(nh, K)
        for name, net in t.networks().items():
            net.load(R.shift_layers(net.export(), 0, ka if "actor" in name else kc)[0])
        ring.rows[:, 4] = R.ldexp32(ring.rows[:, 4].cpu(), K).to(DEV)
    learner = PopulationLearner(td3, rings)
    L, s, tab = lib(), stream_handle(), ptr(learner.table)
    size = len(rings[0])
    out = [dict() for _ in range(P)]
    L.nav_td3_actor_rows_pop(learner.members, P, B, tab, size, 0, s)
    learner._step(1, False, s)
    torch.cuda.synchronize()
    for t, q in zip(td3, out):
        q.update(batch_a=t.batch2.cpu(), masks=[t.mask_a.cpu()], a_q=t.q1.cpu(), a_da=t.da.cpu())
        q.update({f"a_{n}": v.clone() for n, v in R.flat_grad_tensors(
            t.grad_a.cpu(), 2, 2, hidden, t.actor_network.hp, nh).items()})
    L.nav_td3_critic_rows_pop(learner.members, P, B, tab, size, 0, learner.split_twins, s)
    learner._step(0, False, s)
    torch.cuda.synchronize()
    for t, q in zip(td3, out):
        q.update(batch=t.batch.cpu())
        q["masks"] += [t.mask1.cpu(), t.mask2.cpu()]
        for k, (dq, g) in enumerate(((t.dq1, t.grad_c1), (t.dq2, t.grad_c2))):
            q[f"c{k}_dq"], q[f"c{k}_loss"] = dq.cpu(), t.loss_part[k].cpu()
            q.update({f"c{k}_{n}": v.clone() for n, v in R.flat_grad_tensors(
                g.cpu(), 4, 1, hidden, t.critic_network_1.hp, nh).items()})
    return out


def test_population_rows_are_shift_equivariant(nav):
    """nav_td3_critic_rows_pop and nav_td3_actor_rows_pop (with nav_mlp_wgrad_pop and the reduce
    of nav_grad_reduce_adam_pop behind them): member 0 under K = -24 and member 1 under K = +18
    in one launch, each against its own member of an unshifted launch."""
    base, got = _pop_run((None, None)), _pop_run(R.SCALE_KS)
    for m, K in enumerate(R.SCALE_KS):
        exp = dict(critic_shifts(2, K), **actor_shifts(2, K))
        _assert_batch(got[m].pop("batch_a"), base[m].pop("batch_a"), K)
        _assert_epoch(got[m], base[m], exp, K, f"pop member {m} K {K}")


# ---- acting: the actor's internal shifts sum to 0, so nothing may change at all ----
ACTING_SHAPES = [(256, 2), (200, 3)]


def _actor_pair(hidden, nh, seed):
    """(base actor, the same actor with its scale redistributed over its layers: shifts of total
    0, so that the residual it computes is the same f32 value)."""
    from oracle.td3_oracle import make_mlp_params
    p = make_mlp_params(seed, [2] + [hidden] * nh + [2])
    layers = [(torch.tensor(Wl), torch.tensor(b)) for Wl, b in p]
    moved, cums = R.shift_layers(layers, 0, R.joint_shifts(nh, 0)[0])
    assert cums[-1] == 0 and any(c != 0 for c in cums)
    return LN.device_net(layers, 2, 2, hidden, nh), LN.device_net(moved, 2, 2, hidden, nh)


@pytest.mark.parametrize("n", [1, 97])
@pytest.mark.parametrize("hidden,nh", ACTING_SHAPES, ids=_ids(ACTING_SHAPES))
def test_act_ignores_the_layers_scale(nav, hidden, nh, n):
    """nav_act (testing mode): residual and action bit-identical for both actors."""
    from nav._lib import lib, params_struct, ptr, stream_handle
    g = torch.Generator().manual_seed(n + nh)
    st = (torch.rand(n, 2, generator=g, dtype=torch.float64) * 100).to(DEV)
    gl = (torch.rand(n, 2, generator=g, dtype=torch.float64) * 100).to(DEV)
    got = []
    for net in _actor_pair(hidden, nh, 123):
        act = torch.full((n, 2), float("nan"), dtype=torch.float64, device=DEV)
        res = LN.nan(n, 2)
        assert lib().nav_act(C.byref(params_struct()), C.byref(net.desc()), n, ptr(st), ptr(gl),
                             None, None, 0, 1, ptr(act), ptr(res), stream_handle()) == 0
        torch.cuda.synchronize()
        got.append((res.cpu(), act.cpu()))
    assert bool(torch.isfinite(got[0][0]).all()) and bool((got[0][0] != 0).any())
    assert torch.equal(got[1][0], got[0][0]) and torch.equal(got[1][1], got[0][1])


@pytest.mark.parametrize("hidden,nh", ACTING_SHAPES, ids=_ids(ACTING_SHAPES))
def test_act_tick_ignores_the_layers_scale(nav, hidden, nh):
    """nav_act_tick, three training ticks of 97 envs (64-row blocks at any n): actions, rewards,
    replay rows, env state and flags bit-identical for both actors."""
    from nav.vec_env import ReplayRing
    speed, angle = T.random_field(5)
    got = []
    for net in _actor_pair(hidden, nh, 31):
        env = T.make_env(97, speed, angle)
        ring = ReplayRing(1024, DEV)
        action = torch.zeros(97, 2, dtype=torch.float64, device=DEV)
        ticks = []
        for step in range(3):
            r = torch.full((97,), float("nan"), dtype=torch.float64, device=DEV)
            env.act_tick(net, step, ring, action_out=action, reward_out=r)
            ticks += [action.clone(), r]
        torch.cuda.synchronize()
        got.append(ticks + [ring.rows.clone(), env.state.clone(), env.flags.clone()])
    assert bool((got[0][0] != 0).any()) and bool((got[0][-3] != 0).any())
    for i, (u, v) in enumerate(zip(got[1], got[0])):
        assert equal_nan(u, v) if u.is_floating_point() else torch.equal(u, v), i


@pytest.mark.parametrize("hidden,nh", ACTING_SHAPES, ids=_ids(ACTING_SHAPES))
def test_test_rollout_ignores_the_layers_scale(nav, hidden, nh):
    """nav_test_rollout, 97 envs over the full test episode length: the trajectory and every
    output bit-identical for both actors. A whole greedy episode must not notice how the actor's
    scale is distributed over its layers."""
    from nav import config as K
    speed, angle = T.random_field(5)
    env = T.make_env(97, speed, angle)
    start = T.random_starts(env, 9)
    steps = int(K.TEST_TIMEOUT * K.UPDATE_RATE)
    got = []
    for net in _actor_pair(hidden, nh, 31):
        got.append({k: v.cpu() for k, v in env.test_rollout(net, steps, start=start,
                                                            traj=True).items()})
        torch.cuda.synchronize()
    assert got[0].keys() == got[1].keys() and "traj" in got[0]
    assert not torch.equal(got[0]["traj"][0], got[0]["traj"][-1])
    for k in got[0]:
        assert torch.equal(got[1][k], got[0][k]), k


# ---- (5) the ends of the range, against fp64 at the unchanged bars ----
@pytest.mark.parametrize("name,shape,M", R.RANGE_CASES, ids=_ids(R.RANGE_CASES))
def test_range_ends_vs_fp64(nav, name, shape, M):
    """The unfused chain at the range ends of mlp_ref.range_case, where pow2_exp_to's clamp, the
    [-126, 120] clamp of k_wgrad_fact's summed exponent and cap_exp_finite may bind: everything
    finite, every quantity against the fp64 chain of the same f32 data at mlp_ref.bar (2e-6 row
    quantities, 1e-5 cross-row sums, at least 8 * e32), the ReLU bits equal to the fp64 signs
    outside the rounding band. R5: the all-zero tiles' rows of every h_l and dz_l exactly 0."""
    d_in, d_out, hidden, nh = shape
    case = R.range_case(name, d_in, d_out, hidden, nh, M)
    run = R.unfused_chain_run(d_in, d_out, hidden, nh, M, nan_fill=True, case=case)
    layers, x, dy = case
    bits = run["bits"]
    dev = run_quantities(run, shape)
    assert all(bool(torch.isfinite(t).all()) for t in dev.values())
    ref = R.mlp_chain(layers, x, dy, bits)
    # an all-zero row under zero biases and an all-zero weight row give z = 0 exactly in fp64 (R5
    # only): no sign to hold, the bit must be 0, and the entry does not count against the band cap
    live = x.abs().sum(1) > 0
    exact0 = 0
    for z, b in zip(ref["z"], bits):
        assert not bool(b[z == 0].any())
        exact0 += int((z[live] == 0).sum())
    assert exact0 == 0 or name == "R5"
    inside, entries = R.relu_band(layers, x[live], [z[live] for z in ref["z"]],
                                  [b[live] for b in bits])
    R.assert_band_cap(inside - exact0, entries)
    if name == "R5":
        assert not bool(live[R.ZERO_X_ROWS].any()) and int((~live).sum()) == 32
        for l in range(nh):
            assert bool((dev[f"h{l}"][R.ZERO_X_ROWS] == 0).all())
            assert bool((dev[f"dz{l}"][R.ZERO_X_ROWS] == 0).all())
            assert bool((dev[f"dz{l}"][R.ZERO_DY_ROWS] == 0).all())
            assert bool((dev[f"h{l}"][R.ZERO_DY_ROWS] != 0).any())
    f32 = R.mlp_chain(layers, x, dy, bits, torch.float32)
    kind = "crit" if d_out == 1 else "act"
    over = LOG.judge(run["net"].hp, nh, f"{name}_{kind}_{M}",
                     R.compare(dev, R.chain_quantities(ref, nh), R.chain_quantities(f32, nh)))
    assert not over, over
