"""The learner and acting kernels at every hidden width and depth against fp64.

mlp_rows_nt.hip (the launchers of the kernels of rows_kernels.h and td3_rows.h) is compiled once
per NT = hidden_pad / 32 (1 .. 8), each object with an
n_hidden == 1 and an n_hidden >= 2 form and two row-block heights (32-row blocks up to 16 384
rows, 64-row blocks above); the weight gradients fork on shape (k_wgrad_fact / k_wgrad /
k_wgrad_gen). Every form is held here to the project's fp64 bars (tests/mlp_ref.py: row quantities
2e-6 of scale, cross-row sums 1e-5, each at least 8 * e32, e32 the error of an fp32 torch-CPU
evaluation of the same chain): (a) the unfused chain, (b) the fused critic epoch, (c) the fused
actor epoch, (d) the fused reduce + Adam + soft updates, (e) the acting forms. One logical width
per NT, half of them padded, depths 1 .. 4 and the ABI's deepest net (40 x 8).

Every judged figure is printed; with NAV_WIDTH_DEPTH_PARITY=<file> the worst of each (hp,
n_hidden, launch, quantity) is written there at the end of the module (the source of
profiles/width_depth_parity.txt)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import launches as LN
import mlp_ref as R
import pop_support as T
from gpu_support import equal_nan, ids as _ids
from launches import nan as _nan

pytestmark = pytest.mark.gpu
DEV = R.DEV
LOG = R.ParityLog()
BIG = 16421  # 64-row blocks (RT = 2), the last one partial
NAN = float("nan")


@pytest.fixture(scope="module")
def nav():  # this module's own: the teardown writes the parity log
    from nav import _lib
    _lib.require_gpu()
    _lib.lib()
    import nav as navpkg
    yield navpkg
    path = os.environ.get("NAV_WIDTH_DEPTH_PARITY")
    if path:
        LOG.write(path)


# ---- (a) the unfused chain ----
CHAIN_CASES = [(h, nh, k, M) for h, nh in R.SHAPES for k in R.KINDS for M in (1, 33, 97)]
CHAIN_CASES += [(h, 2, k, BIG) for h in (24, 90, 128, 150, 192) for k in R.KINDS]
CHAIN_CASES += [(24, 1, k, BIG) for k in R.KINDS]


@pytest.mark.parametrize("hidden,nh,kind,M", CHAIN_CASES, ids=_ids(CHAIN_CASES))
def test_unfused_chain_vs_fp64(nav, hidden, nh, kind, M):
    """nav_mlp_forward -> nav_mlp_backward -> nav_mlp_wgrad (3 splits) -> nav_grad_reduce: the
    output, every saved activation, every dz row, dx and every tensor of the flat gradient
    against fp64; padded rows and columns exactly 0; NaN-prefilled gradient buffers."""
    d_in, d_out = R.KINDS[kind]
    _, _, d = R.split_gemm_row_errors(d_in, d_out, hidden, nh, M, splits=3, detail=True)
    R.assert_band_cap(*d["band"])
    over = LOG.judge(R.pad32(hidden), nh, f"chain_{kind}", R.compare(d["dev"], d["ref"], d["f32"]))
    assert not over, over


# ---- (b), (c), (d): the fused TD3 epoch ----
def _epoch_setup(hidden, nh, B):
    case = R.epoch_case(hidden, nh, B)
    return (case, *LN.device_epoch(case))


EPOCH_CASES = [(h, nh, B) for h, nh in R.SHAPES for B in (33, 100)] + [(24, 2, BIG), (150, 2, BIG)]


@pytest.mark.parametrize("hidden,nh,B", EPOCH_CASES, ids=_ids(EPOCH_CASES))
def test_fused_critic_epoch_vs_fp64(nav, hidden, nh, B):
    """nav_td3_critic_rows (row backward fused, middle layers saved) -> nav_mlp_wgrad (at
    nav_mlp_wgrad_splits and at 3 splits) -> nav_grad_reduce against the whole of robot.py:329-361
    in fp64 from the f32 weights and rows: batch == rows[idx], dq against 2 (q - y) / B, sum
    (loss_part) / B against the loss, both critics' flat gradients tensor by tensor; split_twins
    0 and 1 bit-identical."""
    from nav._lib import lib
    case, nets, dev = _epoch_setup(hidden, nh, B)
    cr = [nets["cr0"], nets["cr1"]]
    hp = cr[0].hp
    o, o1 = (LN.critic_rows(nets, dev, B, fill=NAN, split=split) for split in (0, 1))
    grads = {}
    for splits in sorted({int(lib().nav_mlp_wgrad_splits(2, 1, hp, nh, B)), 3}):
        for k, g in enumerate(LN.flat_grads(cr, o, splits=splits, fill=NAN)):
            grads[splits, k] = g
    torch.cuda.synchronize()
    for key in ("batch", "lp"):
        assert torch.equal(o[key], o1[key]), key
    for key in ("dq", "es", "masks", "acts", "dz"):  # unsaved layers stay NaN in both
        for k in range(2):
            assert equal_nan(o[key][k].float(), o1[key][k].float()), (key, k)
    batch = case["rows"][case["idx"]]
    assert torch.equal(o["batch"].cpu(), batch)
    bits = [R.relu_bits(o["masks"][k], nh, hp, hidden, B) for k in range(2)]
    (ref, f32), scale = R.critic_refs(case, bits)
    over = []
    for k in range(2):
        R.assert_band_cap(*R.relu_band(case["layers"][f"cr{k}"], batch[:, :4], ref["zs"][k],
                                       bits[k]))
        qr, qf = R.critic_quantities(ref, k), R.critic_quantities(f32, k)
        for splits in sorted({sp for sp, _ in grads}):
            d = dict(dq=o["dq"][k].cpu(), loss=(o["lp"][k].double().sum() / B).reshape(1).cpu())
            d.update(R.flat_grad_tensors(grads[splits, k].cpu(), 4, 1, hidden, hp, nh))
            over += LOG.judge(hp, nh, "critic_rows", R.compare(d, qr, qf, {"dq": scale[k]}))
    assert not over, over


def _actor_rows(nets, dev, B):
    """nav_td3_actor_rows -> nav_mlp_wgrad as TD3.train_actor issues them, NaN-prefilled buffers;
    the reduce's inputs are kept for the update step."""
    o = LN.actor_rows(nets, dev, B, form="plain", fill=NAN)
    return LN.wgrad([nets["actor"]], o, fill=NAN)


@pytest.mark.parametrize("hidden,nh,B", EPOCH_CASES, ids=_ids(EPOCH_CASES))
def test_fused_actor_epoch_vs_fp64(nav, hidden, nh, B):
    """nav_td3_actor_rows -> nav_mlp_wgrad -> nav_grad_reduce against the fp64 gradient of
    -mean Q1(s, pi(s)) (robot.py:382-390) with the kernel's masks_actor and masks_critic bits
    injected: q, da and the actor's flat gradient tensor by tensor.
    The critic's layer-0 input holds pi(s), itself a computed quantity within its bar of the
    reference's, so that layer's kink band is widened by |W0[:, 2:4]| @ (bar_a * max |a|)."""
    case, nets, dev = _epoch_setup(hidden, nh, B)
    actor = nets["actor"]
    hp = actor.hp
    o = LN.actor_rows(nets, dev, B, form="plain", fill=NAN)
    g, = LN.flat_grads([actor], o, fill=NAN)
    torch.cuda.synchronize()
    rows_a = case["rows"][case["idx_a"]]
    assert torch.equal(o["batch"].cpu(), rows_a)
    bits_a = R.relu_bits(o["ma"], nh, hp, hidden, B)
    bits_c = R.relu_bits(o["mc"], nh, hp, hidden, B)
    la, lc = case["layers"]["actor"], case["layers"]["cr0"]
    ref = R.actor_epoch(la, lc, rows_a, bits_a, bits_c)
    f32 = R.actor_epoch(la, lc, rows_a, bits_a, bits_c, torch.float32)
    inside, entries = R.relu_band(la, rows_a[:, :2], ref["zs_a"], bits_a)
    bar_a = R.bar("a", R.rel_err(f32["a"], ref["a"])) * float(ref["a"].abs().max())
    extra = torch.full((1, 2), bar_a, dtype=torch.float64) @ lc[0][0][:, 2:4].double().abs().t()
    i2, e2 = R.relu_band(lc, ref["x_c"], ref["zs_c"], bits_c, extra0=extra)
    R.assert_band_cap(inside + i2, entries + e2)
    d = dict(q=o["q"].cpu(), da=o["da"].cpu())
    d.update(R.flat_grad_tensors(g.cpu(), 2, 2, hidden, hp, nh))
    over = LOG.judge(hp, nh, "actor_rows",
                     R.compare(d, R.actor_quantities(ref), R.actor_quantities(f32)))
    assert not over, over


def _ulp32(x):
    """The f32 spacing at |x| (float64 tensor in, float64 out)."""
    return torch.from_numpy(np.spacing(np.abs(x.numpy()).astype(np.float32)).astype(np.float64))


@pytest.mark.parametrize("hidden", R.WIDTHS)
@pytest.mark.parametrize("nh", [2, 3])
def test_update_step_vs_fp64(nav, hidden, nh):
    """nav_grad_reduce_adam_polyak after the actor epoch's launches against an fp64 restatement of
    torch's Adam (robot.py:236-239) and the soft updates (robot.py:283-285) applied to the
    device's own stored gradient: moments within 1e-6 relative (m relative to its larger operand:
    it is a difference), parameters (from the device's new moments) and targets within 2 ulp of
    f32. The step itself is a chain of f32 roundings (sqrt, two quotients, a sum, a product) that
    an entry smaller than its step does not hide, so an entry's allowance is 2 ulp at its own
    magnitude plus 4 ulp at the step's. Moments start at random values on the logical entries and
    at 0 on the padded ones, which must stay exactly 0."""
    from nav._lib import descs, lib, parr, stream_handle
    L = lib()
    B = 100
    case, nets, dev = _epoch_setup(hidden, nh, B)
    actor, atgt = nets["actor"], nets["atgt"]
    crit, ctgt = [nets["cr0"], nets["cr1"]], [nets["tc0"], nets["tc1"]]
    o = _actor_rows(nets, dev, B)
    logical = R.logical_mask(2, 2, hidden, actor.hp, nh)
    gen = torch.Generator().manual_seed(hidden + nh)
    m0 = torch.randn(actor.count, generator=gen) * 1e-3 * logical
    v0 = torch.rand(actor.count, generator=gen) * 1e-4 * logical
    m, v, g = m0.to(DEV), v0.to(DEV), _nan(actor.count)
    p0, t0 = actor.params.cpu().double(), atgt.params.cpu().double()
    c0 = [t.params.cpu().double() for t in ctgt]
    b1, b2, eps, ss, bc2s, tau = (R.f32c(x) for x in (0.9, 0.999, 1e-8, 1e-3, 0.5, 0.25))
    assert L.nav_grad_reduce_adam_polyak(
        descs(actor), 1, parr(*o["hs"]), o["splits"], parr(o["es"]), o["nblk"], parr(g), parr(m),
        parr(v), b1, b2, eps, (C.c_float * 1)(ss), (C.c_float * 1)(bc2s), descs(atgt),
        descs(*ctgt), descs(*crit), 2, tau, stream_handle()) == 0
    torch.cuda.synchronize()
    gd = g.cpu().double()
    assert bool(torch.isfinite(gd).all()) and bool((gd[~logical] == 0).all())
    b1w = R.f32c(1.0 - b1)
    m1 = m0.double() + b1w * (gd - m0.double())
    v1 = v0.double() * b2 + R.f32c(1.0 - b2) * gd * gd
    md, vd = m.cpu().double(), v.cpu().double()
    # m is a difference of terms of either sign: its rounding is relative to the larger operand
    for name, got, want, mag in (("m", md, m1, torch.maximum(m0.double().abs(), b1w * gd.abs())),
                                 ("v", vd, v1, v1)):
        tol = 1e-6 * torch.maximum(want.abs(), mag)
        err = (got - want).abs()
        assert bool((err <= tol).all()), (name, float((err / tol).nan_to_num().max()))
    # the parameter step from the device's own new moments (f32 values, exact in fp64)
    step = ss * (md / (vd.sqrt() / bc2s + eps))
    p1 = p0 - step
    pd = actor.params.cpu().double()
    assert bool((pd[~logical] == 0).all())
    tol = 2 * _ulp32(torch.maximum(p0.abs(), p1.abs())) + 4 * _ulp32(step)
    assert bool(((pd - p1).abs() <= tol).all()), float(((pd - p1).abs() / tol).max())
    omt = R.f32c(1.0 - tau)
    for name, net, old, src in (("actor", atgt, t0, pd), ("critic1", ctgt[0], c0[0], crit[0]),
                                ("critic2", ctgt[1], c0[1], crit[1])):
        src = src if torch.is_tensor(src) else src.params.cpu().double()
        want = old * omt + src * tau
        tol = 2 * _ulp32(torch.maximum(torch.maximum(old.abs(), want.abs()), src.abs() * tau))
        err = (net.params.cpu().double() - want).abs()
        assert bool((err <= tol).all()), (name, float((err / tol).nan_to_num().max()))
    R._assert_images_exact(actor, "reduce_adam")
    R._assert_images_exact(atgt, "own_target")


# ---- (e) the acting forms: one depth per width, cycling 1 .. 4 ----
ACTING = [(h, 1 + i % 4) for i, h in enumerate(R.WIDTHS)]


@pytest.mark.parametrize("n", [1, 97])
@pytest.mark.parametrize("hidden,nh", ACTING, ids=_ids(ACTING))
def test_act_residual_vs_fp64(nav, hidden, nh, n):
    """nav_act's testing-mode residual (robot.py:598-624) against the fp64 forward of
    f32(state - goal)."""
    from nav._lib import lib, params_struct, ptr, stream_handle
    net, layers = R.make_net(2, 2, hidden, nh, 123)
    g = torch.Generator().manual_seed(n + nh)
    st = torch.rand(n, 2, generator=g, dtype=torch.float64) * 100
    gl = torch.rand(n, 2, generator=g, dtype=torch.float64) * 100
    std, gld = st.to(DEV), gl.to(DEV)
    act = torch.zeros(n, 2, dtype=torch.float64, device=DEV)
    res = _nan(n, 2)
    assert lib().nav_act(C.byref(params_struct()), C.byref(net.desc()), n, ptr(std), ptr(gld),
                         None, None, 0, 1, ptr(act), ptr(res), stream_handle()) == 0
    torch.cuda.synchronize()
    x = (st - gl).float()
    ref, f32 = R.mlp_forward(layers, x)[0], R.mlp_forward(layers, x, torch.float32)[0]
    over = LOG.judge(net.hp, nh, "act", R.compare(dict(residual=res.cpu()), dict(residual=ref),
                                                  dict(residual=f32)))
    assert not over, over


@pytest.mark.parametrize("hidden,nh", ACTING, ids=_ids(ACTING))
def test_act_tick_is_bit_identical(nav, hidden, nh):
    """nav_act_tick against nav_act + nav_agent_step over 4 training steps of two equal
    trainers: actions, rewards, next states, goal terms, block stats, replay rows, env state,
    flags and the learner, bit for bit (the recipe of test_fused_act_tick_is_bit_identical)."""
    from nav.trainer import VecTrainer
    runs = []
    for fused in (True, False):
        tr = VecTrainer(n_envs=192, hidden=hidden, n_hidden=nh, batch=64, updates_per_step=2,
                        demos=False, device=DEV)
        got = []
        for _ in range(4):
            r = torch.full((tr.n,), float("nan"), dtype=torch.float64, device=DEV)
            if fused:
                tr.env.act_tick(tr.td3.actor_network, tr.steps, tr.replay, action_out=tr.action,
                                reward_out=r)
            else:
                tr.act()
                tr.env.agent_step(tr.action, tr.replay, reward_out=r)
            tr.steps += 1
            tr.learn()
            got.append((tr.action.clone(), r, tr.env.next_state.clone(), tr.env.goal_term.clone(),
                        tr.env.block_stats.clone()))
        torch.cuda.synchronize()
        runs.append((tr, got))
    (a, ga), (b, gb) = runs
    assert torch.equal(a.replay.rows, b.replay.rows)
    assert torch.equal(a.env.state, b.env.state)
    assert torch.equal(a.env.flags, b.env.flags)
    for t, (x, y) in enumerate(zip(ga, gb)):
        for i, (u, v) in enumerate(zip(x, y)):
            assert equal_nan(u, v), (t, i)
    for k, net in a.td3.networks().items():
        assert torch.equal(net.params, b.td3.networks()[k].params), k


@pytest.mark.parametrize("hidden,nh", ACTING, ids=_ids(ACTING))
def test_test_rollout_is_bit_identical(nav, orc, hidden, nh):
    """nav_test_rollout over 97 envs and 8 steps against the host loop of nav_act(mode 1) ->
    nav_env_step it fuses (tests/test_gpu_test_rollout.py), bit for bit."""
    speed, angle = T.random_field(5)
    env = T.make_env(97, speed, angle)
    actor, _ = T.make_actor(hidden, nh, 31)
    start = T.random_starts(env, 9)
    got = T.clone_out(env.test_rollout(actor, 8, start=start, traj=True))
    torch.cuda.synchronize()
    ref = T.unfused_episode(orc, env, actor, start, 8)
    assert torch.equal(got["traj"], ref["traj"])
    assert torch.equal(got["final_state"], ref["final_state"])
    for k in ("reached", "steps", "best_distance"):
        assert torch.equal(got[k].cpu(), ref[k]), k
