"""The row kernels and the acting launches at the bench's grid size against independent references.

The bench's collect launch runs 1 024 workgroups of 64 rows: four per CU on a 256-CU MI355X, in
four bands of 256 that alternate the `favored` GEMM priority path ((blockIdx.x / kCUs) & 1 in
gemm_cols / gemm_bits). The fp64 checks elsewhere stop at 16 421 rows (257 workgroups: one CU
holds a co-resident pair); here every band is occupied and every 64-row block is held to the same
bound on its own, so a failure names the block and its band."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden
from gpu_support import nav  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = (0x5A17 << 32) | 424242  # seed_hi != 0


def _assert_blocks(name, err, scale, bound):
    """Every 64-row block's worst |err| / scale within `bound`; the message names the worst
    failing block, its band of 256 blocks and the failing rows' residues mod 8."""
    M = err.numel()
    e = torch.cat([err, err.new_zeros(-M % 64)]).view(-1, 64) / scale
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    worst = e.amax(1)
    bad = torch.nonzero(worst > bound).view(-1)
    if len(bad):
        b = int(bad[worst[bad].argmax()])
        rows = torch.nonzero(e.view(-1)[:M] > bound).view(-1)
        raise AssertionError(
            f"{name}: {len(bad)} of {len(worst)} blocks over {bound:g}; worst block {b} (band "
            f"{b // 256}) at {float(worst[b]):.3e}; failing blocks per band "
            f"{torch.bincount(bad // 256, minlength=4).tolist()}; failing rows mod 8 "
            f"{torch.bincount(rows % 8, minlength=8).tolist()}")
    return float(worst.max())


# M = 65 505: 1 024 workgroups of 64 rows, the last one holding 33 rows (one full 32-row tile and
# a one-row tile)
@pytest.mark.parametrize("d_in,d_out,hidden,nh", [(2, 2, 256, 2), (4, 1, 256, 2), (2, 2, 200, 3)])
def test_row_kernels_vs_fp64_every_band_occupied(nav, d_in, d_out, hidden, nh):
    """nav_mlp_forward, nav_mlp_backward and the weight gradients at 65 505 rows against the fp64
    reference of test_split_gemm_f32_accuracy_vs_fp64 (same helper, same bounds): outputs, saved
    activations, dz and dx within 2e-6 of scale in every 64-row block, dW within 1e-5, ReLU bits
    equal to the fp64 signs outside the rounding band.
    Measured on MI355X, worst block of (2,2,256,2) / (4,1,256,2) / (2,2,200,3):
    out 3.2e-7 / 3.4e-7 / 6.2e-7, h 1.0e-7 .. 5.3e-7, dz 4.2e-8 .. 3.7e-7, dx 4.7e-7 / 3.8e-7 /
    3.6e-7 of scale (fp32 itself ~1e-7), dW 8.3e-7 / 5.9e-7 / 6.8e-7; no band stands out."""
    from nav._lib import lib
    from mlp_ref import split_gemm_row_errors
    M = 65505
    assert lib().nav_mlp_row_blocks(M) == 1024
    rows, dW = split_gemm_row_errors(d_in, d_out, hidden, nh, M)
    print({k: f"{float(e.max()) / s:.2e}" for k, (e, s) in rows.items()},
          {k: f"{v:.2e}" for k, v in dW.items()})
    for k, (e, s) in rows.items():
        _assert_blocks(k, e, s, 2e-6)
    for k, v in dW.items():
        assert v <= 1e-5, (k, v)


@pytest.fixture(scope="module")
def acting(nav):
    """A 256 x 2 actor over 65 536 envs (1 024 workgroups) with random states and goals in the
    world and per-env noise scales in [0.05, 0.5]; nav_act's training and testing launches at
    step 7, and the fp64 forward of f32(state - goal)."""
    from nav._lib import lib, params_struct, ptr, stream_handle
    from nav.vec_env import VecEnv, make_field
    from mlp_ref import _f64_forward, make_net
    t = golden("trace.npz")
    n, step = 65536, 7
    env = VecEnv(n, make_field(t["speed"], t["angle"], DEV), seed=SEED, envs_per_group=1024)
    g = torch.Generator().manual_seed(31)
    st = torch.rand(n, 2, generator=g, dtype=torch.float64) * 98.9
    gl = torch.rand(n, 2, generator=g, dtype=torch.float64) * 90 + 5
    sc = torch.rand(n, generator=g, dtype=torch.float64) * 0.45 + 0.05
    # every other env's goal within 4 of its state per axis: |state - goal| of two random points
    # is mostly over max_action, and a clipped action shows neither the residual nor the noise
    near = torch.rand(n, 2, generator=g, dtype=torch.float64) * 8 - 4
    gl[1::2] = (st[1::2] + near[1::2]).clamp(5, 95)
    env.state.copy_(st); env.goal.copy_(gl); env.noise_scale.copy_(sc)
    net, layers = make_net(2, 2, 256, 2, 123)
    p = params_struct(seed_lo=SEED & 0xFFFFFFFF, seed_hi=SEED >> 32)
    out = {}
    for mode, key in ((0, "train"), (1, "test")):
        act = torch.full((n, 2), float("nan"), dtype=torch.float64, device=DEV)
        res = torch.full((n, 2), float("nan"), device=DEV)
        assert lib().nav_act(C.byref(p), C.byref(net.desc()), n, ptr(env.state), ptr(env.goal),
                             ptr(env.noise_scale), None, step, mode, ptr(act), ptr(res),
                             stream_handle()) == 0
        torch.cuda.synchronize()
        out[key] = (act.cpu().numpy(), res.cpu().numpy())
    ref, _ = _f64_forward(layers, (st - gl).float())
    return dict(env=env, net=net, n=n, step=step, st=st.numpy(), gl=gl.numpy(), sc=sc.numpy(),
                ref=ref, **out)


def _epilogue(a, res, z):
    """orc_act_epilogue (robot.py:556-567 / 586-593) over all envs in numpy: the same f64
    operations in the same order."""
    c = (a["st"] - a["gl"]) + res.astype(np.float64)
    if z is not None:
        c = c + (a["sc"] * 5.0)[:, None] * z
    return np.clip(c, -5.0, 5.0)


def test_act_residual_and_noise_vs_oracle_at_bench_grid(acting, orc):
    """nav_act at 65 536 rows, training mode, noise from Philox (seed_hi != 0, step 7): the
    residual against the fp64 forward within 2e-6 of scale in every 64-row block, the action
    against orc_act_epilogue of (state, goal, the device's residual, sigma, oracle.vec_noise)
    within 1e-11 (f64 device math against libm: only Box-Muller's log / sincos differ); testing
    mode exactly the epilogue of its residual.
    Measured on MI355X: residual worst block 2.9e-7 of scale, action max |diff| 1.8e-15, 47 % of
    the action entries clipped."""
    a = acting
    p = orc.default_params(SEED)
    act, res = a["train"]
    worst = _assert_blocks("residual", (torch.tensor(res).double() - a["ref"]).abs().amax(1),
                           float(a["ref"].abs().max()), 2e-6)
    z = orc.vec_noise(p, a["n"], a["step"])
    want = _epilogue(a, res, z)
    # the vectorised epilogue is the oracle's, value for value
    for e in range(0, a["n"], 97):
        assert np.array_equal(want[e], orc.act_epilogue(a["st"][e], a["gl"][e], res[e],
                                                        a["sc"][e], z[e])), e
    d = np.abs(act - want)
    print(f"residual worst block {worst:.2e} of scale; action max |diff| {d.max():.2e}; "
          f"clipped {np.mean(np.abs(want) == 5.0):.3f}")
    assert np.isfinite(act).all() and d.max() <= 1e-11, int(d.max(1).argmax())
    assert 0.05 < np.mean(np.abs(want) == 5.0) < 0.95  # both sides of the clip are exercised
    # the noise is in the action: without it the same epilogue is far off
    assert np.abs(act - _epilogue(a, res, None)).max() > 1.0
    act_t, res_t = a["test"]
    assert np.array_equal(res_t, res)
    assert np.array_equal(act_t, _epilogue(a, res_t, None))
    for e in range(0, a["n"], 97):
        assert np.array_equal(act_t[e], orc.act_epilogue(a["st"][e], a["gl"][e], res_t[e],
                                                         a["sc"][e], None)), e


def test_branch_trace_at_bench_grid(nav):
    """The indexed reward path (nav_agent_step_indexed) at the bench's grid: 65 536 envs, every
    one replaying the reference's branch trace (trace_branches.npz: goal, path end, stuck and
    their coincidences, NaN actions, steps clipped at a world edge). At every step tick env 0's
    flags, next state and replay row are held to the reference's record with
    test_agent_step_replays_reference_trace's bounds, and every other env's flags, next state,
    counters and row equal env 0's bit for bit (one comparison on the device per tick), so a
    workgroup or band that forms a branch differently shows."""
    from nav.vec_env import ReplayRing, VecEnv, make_field
    from trace_support import check_goal_row, step_ticks, want_flags
    t = golden("trace_branches.npz")
    n = 65536
    env = VecEnv(n, make_field(t["speed"], t["angle"], DEV), envs_per_group=n, init=False)
    first, ticks = step_ticks(t)
    c = t["counters"]
    env.state.copy_(torch.tensor(t["tick_state"][first]).expand(n, 2))
    env.goal.copy_(torch.tensor(t["goal"]).expand(n, 2))
    env.region.copy_(torch.tensor(t["region"]).expand(n, 4))
    env.plan_index.fill_(int(c[first][0]))
    env.path_length.fill_(int(c[first][1]))
    env.episodes.fill_(int(c[first][2]))
    env.noise_scale.fill_(float(c[first][6]))
    env.meta.fill_(4)
    env.set_demo(t["demo_set"])
    assert env.fuse_demo and env.demo_index is not None
    rep = ReplayRing(n, DEV)
    bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64)  # noqa: E731
    for i, lo, reset_state in ticks:
        a = torch.tensor(t["tick_action"][i], device=DEV).expand(n, 2).contiguous()
        base = env.agent_step(a, rep)
        assert base == 0
        same = [torch.equal(env.flags, env.flags[:1].expand(n)),
                torch.equal(bits(env.next_state), bits(env.next_state[:1]).expand(n, 2)),
                torch.equal(bits(rep.rows), bits(rep.rows[:1]).expand(n, 8)),
                torch.equal(env.plan_index, env.plan_index[:1].expand(n)),
                torch.equal(env.path_length, env.path_length[:1].expand(n)),
                torch.equal(env.episodes, env.episodes[:1].expand(n)),
                torch.equal(env.meta, env.meta[:1].expand(n)),
                torch.equal(bits(env.noise_scale), bits(env.noise_scale[:1]).expand(n))]
        assert all(same), (i, same)
        fl = int(env.flags[0].item())
        row = rep.rows[0].cpu().numpy()
        ref_r = t["push_r"][lo]
        assert (fl & 15) == want_flags(t, i, lo, reset_state), (i, fl)
        assert abs(float(row[4]) - ref_r) <= 1e-5 * max(1.0, abs(ref_r)), i
        check_goal_row(t, i, lo, row[4])
        assert np.max(np.abs(env.next_state[0].cpu().numpy() - t["push_s2"][lo])) < 1e-11
        if reset_state is not None:
            assert env.episodes[0].item() == int(c[i + 1][2])
            assert env.path_length[0].item() == int(c[i + 1][1])
            # every env drew its own reset state: all of them within the region, then the
            # reference's draw for all
            reg = t["region"]
            s = env.state
            assert bool(((s[:, 0] >= reg[0]) & (s[:, 0] <= reg[1]) & (s[:, 1] >= reg[2]) &
                         (s[:, 1] <= reg[3])).all()), i
            env.state.copy_(torch.tensor(reset_state).expand(n, 2))
        else:
            assert torch.equal(bits(env.state), bits(env.state[:1]).expand(n, 2)), i


def test_act_tick_action_equals_act_at_bench_grid(acting):
    """nav_act_tick's action_out on the same state equals nav_act's bit for bit at four
    workgroups per CU (the fused launch draws the same noise and forms the same epilogue)."""
    from nav.vec_env import ReplayRing
    a = acting
    env = a["env"]
    rep = ReplayRing(a["n"], DEV)
    out = torch.full((a["n"], 2), float("nan"), dtype=torch.float64, device=DEV)
    env.act_tick(a["net"], a["step"], rep, action_out=out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), a["train"][0])
    # the tick consumed those actions: they are the replay rows' action columns
    assert torch.equal(rep.rows[:, 2:4], out.float())
