"""nav_test_rollout / VecEnv.test_rollout / VecTrainer.evaluate: whole greedy test episodes
(robot-learning.py:78, 104-117) of every env in one launch, against the two-launch composition it
fuses (bit for bit), against its own trajectory, against the CPU oracle step by step and over
whole episodes, its start draw, and its promise to leave the trainer untouched."""
import numpy as np
import pytest
import torch

from gpu_support import nav  # noqa: F401
from pop_support import (DEV, clone_out, equal_tree as _equal_tree, make_actor, make_env,
                         norm2_rows, random_field, random_starts, unfused_episode)

pytestmark = pytest.mark.gpu
T_BITS = 12  # steps of the bitwise cases
_cases = {}


def bit_case(orc, hidden, nh, n):
    """(env, actor, start, the kernel's outputs, the unfused loop's): computed once per shape."""
    key = (hidden, nh, n)
    if key not in _cases:
        speed, angle = random_field(5)
        env = make_env(n, speed, angle)
        actor, layers = make_actor(hidden, nh, 31)
        start = random_starts(env, 9)
        got = clone_out(env.test_rollout(actor, T_BITS, start=start, traj=True))
        torch.cuda.synchronize()
        ref = unfused_episode(orc, env, actor, start, T_BITS)
        _cases[key] = dict(env=env, actor=actor, layers=layers, start=start, got=got, ref=ref,
                           speed=speed, angle=angle)
    return _cases[key]


@pytest.mark.parametrize("n", [1, 97, 16421])
@pytest.mark.parametrize("hidden,nh", [(200, 3), (256, 2)])
def test_bitwise_vs_unfused_composition(nav, orc, hidden, nh, n):
    """traj, final_state, reached, steps and best_distance equal the host loop of nav_act(mode=1)
    -> nav_env_step bit for bit: one-row tile, partial tile, and the 64-row side of the block
    height switch."""
    c = bit_case(orc, hidden, nh, n)
    got, ref = c["got"], c["ref"]
    if n > 1:
        # a condition on the inputs: some rows stop early, some run to the end
        r = ref["reached"]
        assert 0 < int(r.sum()) < n
        assert int((ref["steps"] == 1).sum()) > 0
    assert torch.equal(got["traj"], ref["traj"])
    assert torch.equal(got["final_state"], ref["final_state"])
    assert torch.equal(got["reached"].cpu(), ref["reached"])
    assert torch.equal(got["steps"].cpu(), ref["steps"])
    assert torch.equal(got["best_distance"].cpu(), ref["best_distance"])


def test_outputs_are_what_traj_implies(nav, orc):
    """reached / steps / best_distance / final_state recomputed on the CPU from traj and the
    goals (orc.norm2, the threshold of params_struct()): equal, the doubles bit for bit."""
    from nav._lib import params_struct
    c = bit_case(orc, 200, 3, 97)
    got = {k: v.cpu().numpy() for k, v in c["got"].items()}
    goal = c["env"].goal.cpu().numpy()
    thr = params_struct().goal_threshold
    traj = got["traj"]
    T, n = traj.shape[:2]
    for e in range(n):
        dist = norm2_rows(orc, traj[:, e] - goal[e])
        hits = np.nonzero(dist <= thr)[0]
        k = int(hits[0]) + 1 if len(hits) else T  # steps taken
        assert got["reached"][e] == (1 if len(hits) else 0)
        assert got["steps"][e] == k
        assert got["best_distance"][e] == dist[:k].min()
        assert np.array_equal(got["final_state"][e], traj[k - 1, e])
        assert np.array_equal(traj[k - 1:, e], np.broadcast_to(traj[k - 1, e], (T - k + 1, 2)))


def test_teacher_forced_step_parity(nav, orc):
    """Every step of every env against an independent CPU step from the kernel's own previous
    state: torch-CPU fp32 forward of f32(s - goal), orc.act_epilogue, orc.step; |traj[t] - next|
    <= 3e-4 per component. The bound is derived: the action is pinned at 2e-4 per component
    (test_act_vs_reference_golden), speed < 1 and a rotation turn that into at most 2e-4 * sqrt(2)
    < 3e-4 of displacement. The n = 97 case's field, goals, starts and actor with goal_threshold 0,
    so that no env stops and every (step, env) is a real step. Measured maximum on an MI355X:
    see DESIGN.md (test episodes)."""
    c = bit_case(orc, 200, 3, 97)
    T, n = 8, 97
    env = make_env(n, c["speed"], c["angle"], goal_threshold=0.0)
    assert torch.equal(env.goal, c["env"].goal)
    out = env.test_rollout(c["actor"], T, start=c["start"], traj=True)
    traj = out["traj"].cpu().numpy()
    assert int(out["reached"].sum()) == 0
    goal = env.goal.cpu().numpy()
    prev = c["start"].cpu().numpy()
    worst = 0.0
    for t in range(T):
        x = torch.tensor((prev - goal).astype(np.float32))
        h = x
        for i, (W, b) in enumerate(c["layers"]):
            h = torch.nn.functional.linear(h, W, b)
            if i < len(c["layers"]) - 1:
                h = torch.relu(h)
        res = h.numpy()
        for e in range(n):
            a = orc.act_epilogue(prev[e], goal[e], res[e], 0, None)
            nxt, _ = orc.step(c["speed"], c["angle"], prev[e], a)
            worst = max(worst, float(np.abs(traj[t, e] - nxt).max()))
        prev = traj[t]
    print(f"teacher-forced max |traj - next| = {worst:.3e}")
    assert worst <= 3e-4


def test_homing_episode_vs_cpu_rollout(nav, orc):
    """Constant field (speed 1, angle 0.5: rot = f32 pi, the baseline action points at the goal),
    an all-zero actor (residual exactly 0), one goal, starts on a spiral: every env walks home in
    1 to 17 steps, whole tiles leave early while row 96 runs on. Step counts exact, states and
    best distances within 1e-9 of the CPU rollout (device dynamics is pinned to the oracle at
    1e-11 per step)."""
    from nav.mlp import DeviceMLP
    n = 97
    speed = np.full((100, 100), 1.0, np.float32)
    angle = np.full((100, 100), 0.5, np.float32)
    env = make_env(n, speed, angle)
    g = np.array([8.0, 9.0])
    env.goal.copy_(torch.tensor(g).expand(n, 2))
    i = np.arange(n)
    r, th = 5.5 + 0.85 * i, 0.1 + 1.3 * i / 96
    start = g + r[:, None] * np.stack([np.cos(th), np.sin(th)], 1)
    actor = DeviceMLP(2, 2, 64, 2, DEV)  # all parameters zero
    actor.pack()
    # the CPU rollout
    dists, finals = [], []
    margin = np.inf
    for e in range(n):
        s, ds = start[e].copy(), []
        for _ in range(64):
            s, _ = orc.step(speed, angle, s, np.clip(s - g, -5.0, 5.0))
            ds.append(orc.norm2(s[0] - g[0], s[1] - g[1]))
            margin = min(margin, abs(ds[-1] - 5.0))
            if ds[-1] <= 5.0:
                break
        assert ds[-1] <= 5.0
        dists.append(ds)
        finals.append(s)
    steps = np.array([len(d) for d in dists], np.int32)
    # conditions on the inputs: no distance near the threshold, early tiles, a late row
    assert margin > 1e-6
    assert steps.min() == 1 and steps.max() == 17
    assert steps[:32].max() <= 5 and steps[:64].max() <= 9 and steps[96] == 17
    st = torch.tensor(start, device=DEV)
    out = clone_out(env.test_rollout(actor, 24, start=st))
    assert torch.all(out["reached"] == 1)
    assert np.array_equal(out["steps"].cpu().numpy(), steps)
    assert np.abs(out["final_state"].cpu().numpy() - np.array(finals)).max() <= 1e-9
    out = clone_out(env.test_rollout(actor, 6, start=st))
    want = steps <= 6
    assert int(want.sum()) == 50
    assert np.array_equal(out["reached"].cpu().numpy().astype(bool), want)
    assert np.array_equal(out["steps"].cpu().numpy(), np.where(want, steps, 6))
    best = np.array([min(d[:6]) for d in dists])
    assert np.abs(out["best_distance"].cpu().numpy() - best).max() <= 1e-9


def test_teacher_forced_by_the_reference(nav):
    """One launch, one env per (episode, step) pair the reference recorded in its own testing
    loop (test_episodes.npz group a: robot-learning.py:104-117 on a make_fields field with a
    generator-defined 2-200-200-200-2 actor): start = the reference's state at that step, goal =
    the episode's, max_steps = 1. Every next state within 3e-4 per component of the reference's
    (test_teacher_forced_step_parity's derived bound), reached == (distance <= 5) for EVERY pair
    (the fixture keeps every distance 1e-3 from the threshold), best_distance within
    3e-4 * sqrt(2) of the recorded distance. 209 pairs: three full tiles and a tail.
    Measured maximum on an MI355X: see DESIGN.md (test episodes)."""
    from conftest import golden
    g = golden("test_episodes.npz")
    n = len(g["a_ep"])
    assert n % 64 != 0
    env = make_env(n, g["a_speed"], g["a_angle"])
    env.goal.copy_(torch.tensor(g["a_goal"][g["a_ep"]]))
    actor, _ = make_actor(200, 3, int(g["a_actor_seed"]))
    start = torch.tensor(g["a_state"], device=DEV)
    out = {k: v.cpu().numpy() for k, v in env.test_rollout(actor, 1, start=start,
                                                           traj=True).items()}
    err = np.abs(out["traj"][0] - g["a_next"])
    derr = np.abs(out["best_distance"] - g["a_dist"])
    print(f"teacher-forced by the reference: max |next - ref| = {err.max():.3e}, "
          f"max |best_distance - ref| = {derr.max():.3e} over {n} pairs")
    assert err.max() <= 3e-4, int(err.max(1).argmax())
    want = g["a_dist"] <= 5.0
    assert 0 < want.sum() < n
    assert np.array_equal(out["reached"].astype(bool), want)
    assert derr.max() <= 3e-4 * np.sqrt(2.0)
    assert (out["steps"] == 1).all()
    assert np.array_equal(out["final_state"], out["traj"][0])


def _reference_closed_loop(g, cap):
    """Per episode of group (b), what the reference's testing loop gave under a cap of `cap`
    steps: steps taken, reached, the final state, and the best distance over the steps taken.
    For an episode that did not reach the goal that is the reference's own test_best_distance
    (asserted here); for one that did, the reference exits before its `<` update
    (robot-learning.py:110-114) and never reports the variable, so the minimum includes the
    reaching step's recorded distance, as nav_test_rollout documents."""
    from trace_support import episode_slices
    steps, reached, final, best = [], [], [], []
    for e, ix in enumerate(episode_slices(g, "b_")):
        k = min(len(ix), cap)
        hit = len(ix) <= cap
        d = g["b_dist"][ix][:k]
        steps.append(k)
        reached.append(hit)
        final.append(g["b_next"][ix][k - 1])
        best.append(d.min())
        ref_best = g["b_best"][e] if cap >= int(g["b_cap"]) else g["b6_best"][e]
        if not hit:
            assert d.min() == ref_best
        else:
            assert (g["b_reached_step"][e], d[-1] <= 5.0) == (k, True)
            assert ref_best == (d[:-1].min() if k > 1 else np.inf)
    if cap == 6:
        assert np.array_equal(np.array(steps), g["b6_steps"])
        assert np.array_equal(np.array(reached), g["b6_reached_step"] > 0)
        assert np.array_equal(np.array(final), g["b6_final"])
    return (np.array(steps, np.int32), np.array(reached), np.array(final), np.array(best))


@pytest.mark.parametrize("form", ["single", "pop"])
def test_closed_loop_vs_reference_episodes(nav, form):
    """Whole test episodes against the reference's own (test_episodes.npz group b: the constant
    field, an all-zero actor, one goal, 25 starts on a spiral, 1 to 17 steps): steps and reached
    equal for every episode at a cap past the longest episode and at the cap of 6, final_state
    and best_distance within 1e-9 (the device dynamics is pinned at 1e-11 per step). `pop`: the
    same through nav_test_rollout_pop, the episodes split over 2 members holding equal actors
    (a member holds a multiple of 64 envs: the 25 episodes repeated to fill 2 x 64)."""
    from conftest import golden
    from nav.mlp import DeviceMLP
    g = golden("test_episodes.npz")
    E = len(g["b_goal"])
    sel = np.arange(E) if form == "single" else np.arange(128) % E
    n = len(sel)
    speed = np.full((100, 100), 1.0, np.float32)
    angle = np.full((100, 100), 0.5, np.float32)
    env = make_env(n, speed, angle)
    env.goal.copy_(torch.tensor(g["b_goal"][sel]))
    st = torch.tensor(g["b_start"][sel], device=DEV)
    actors = [DeviceMLP(2, 2, 64, 2, DEV) for _ in range(2)]  # all parameters zero
    for a in actors:
        a.pack()
    if form == "pop":
        from nav.population import PopulationTable
        pop = PopulationTable(actors, [env.p, env.p], None, n // 2)
    seen = []
    for cap in (int(g["b_cap"]), 6):
        steps, reached, final, best = _reference_closed_loop(g, cap)
        assert steps.max() <= cap
        out = env.test_rollout(actors[0], cap, start=st) if form == "single" else \
            env.test_rollout_pop(pop, cap, start=st)
        out = {k: v.cpu().numpy() for k, v in out.items()}
        assert np.array_equal(out["steps"], steps[sel])
        assert np.array_equal(out["reached"].astype(bool), reached[sel])
        assert np.abs(out["final_state"] - final[sel]).max() <= 1e-9
        assert np.abs(out["best_distance"] - best[sel]).max() <= 1e-9
        seen.append((int(reached.sum()), int((~reached).sum())))
    assert seen[0] == (E, 0) and min(seen[1]) >= 5  # all reach; the cap of 6 cuts 12 off


def test_start_draw(nav, orc):
    """start = NULL: env e starts at region_sample(region[e], u01(w.x, w.y), u01(w.z, w.w)), w =
    philox(0, e, NAV_TAG_TEST = 6, episode): the first step equals the explicit-start run from the
    CPU-derived starts bit for bit; the same episode repeats, another episode starts elsewhere."""
    c = bit_case(orc, 200, 3, 97)
    env, actor = c["env"], c["actor"]
    region = env.region.cpu().numpy()

    def u01(hi, lo):  # nav_device.h:38-40
        return (float(hi >> 5) * 67108864.0 + float(lo >> 6)) / 9007199254740992.0

    def starts(episode):
        out = np.zeros((env.n, 2))
        for e in range(env.n):
            w = orc.philox([0, e, 6, episode], [env.p.seed_lo, env.p.seed_hi])
            out[e] = orc.reset_u(region[e], u01(w[0], w[1]), u01(w[2], w[3]))
        return out

    firsts = {}
    for episode in (0, 3):
        drawn = clone_out(env.test_rollout(actor, 1, episode=episode, traj=True))
        s0 = starts(episode)
        assert np.all((s0[:, 0] >= region[:, 0]) & (s0[:, 0] <= region[:, 1]))
        given = clone_out(env.test_rollout(actor, 1, start=torch.tensor(s0, device=DEV),
                                           traj=True))
        for k in drawn:
            assert torch.equal(drawn[k], given[k]), k
        again = env.test_rollout(actor, 1, episode=episode, traj=True)
        for k in drawn:
            assert torch.equal(drawn[k], again[k]), k
        firsts[episode] = (s0, drawn["traj"][0].cpu().numpy())
    assert np.all(np.any(firsts[0][0] != firsts[3][0], axis=1))
    assert np.any(firsts[0][1] != firsts[3][1])


def test_evaluate_leaves_training_untouched(nav):
    """Two equal trainers, 3 steps each, evaluate() on one, 2 more steps each: equal state_dicts.
    evaluate() returns the documented dict; its success_rate is the mean of a direct
    test_rollout's reached flags."""
    from nav.trainer import VecTrainer

    def trainer():
        return VecTrainer(n_envs=256, hidden=64, n_hidden=2, batch=128, demos=False, seed=1234,
                          device=DEV)

    a, b = trainer(), trainer()
    for _ in range(3):
        a.step()
        b.step()
    ev = a.evaluate(max_steps=16)
    assert set(ev) == {"n", "success_rate", "mean_steps_reached", "mean_best_distance",
                       "max_best_distance", "max_steps", "episode"}
    assert (ev["n"], ev["max_steps"], ev["episode"]) == (256, 16, 0)
    direct = a.env.test_rollout(a.td3.actor_network, 16, episode=0)
    assert ev["success_rate"] == direct["reached"].float().mean().item()
    assert ev["max_best_distance"] == direct["best_distance"].max().item()
    assert ev["mean_best_distance"] <= ev["max_best_distance"]
    for _ in range(2):
        a.step()
        b.step()
    torch.cuda.synchronize()
    _equal_tree(a.state_dict(), b.state_dict())
