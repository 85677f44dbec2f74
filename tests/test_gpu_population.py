"""Population launches (nav_act_tick_pop, nav_test_rollout_pop) and PopulationTrainer against the
single-policy launches they generalise, bit for bit: envs do not interact, so member m's envs must
end exactly as they do when nav_act_tick / nav_test_rollout runs over the WHOLE env set with
member m's actor and constants from the same starting state, read on member m's slice. No
tolerance anywhere."""
import numpy as np
import pytest
import torch

from conftest import golden
from gpu_support import nav  # noqa: F401
from pop_support import (SOA, clone_out, equal_tree as _equal_tree, make_actor, member_state,
                         random_field, random_starts)

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, EPM, EPG = 3, 128, 64
N = P * EPM
TICKS = 40
T_TEST = 12
SEED = 77
STEP_OUT = ("next_state", "goal_term", "flags", "block_stats")


def member_params(m, distinct=True, **extra):
    """Member m's constants: the fields a member may set for itself all differ between members;
    path_length0 = 6 for all, so episodes end and auto-reset inside a 40-tick run."""
    from nav._lib import params_struct
    kw = dict(seed_lo=SEED, seed_hi=0, path_length0=6)
    if distinct:
        kw.update(demo_factor=10.0 + 20.0 * m, noise_decay=0.75 - 0.2 * m,
                  stuck_penalty=50.0 - 15.0 * m, goal_reward=50.0 + 25.0 * m,
                  path_increase=20 - 7 * m)
    kw.update(extra)
    return params_struct(**kw)


def make_env(n, demos, field=None):
    """n envs in groups of EPG, path_length0 = 6; demos: each group's demo set is a shifted copy
    of the reference demonstration set, indexed."""
    from nav.vec_env import VecEnv, make_field
    env = VecEnv(n, field if field is not None else make_field(*random_field(5), DEV), seed=SEED,
                 envs_per_group=EPG, demo_flag=demos, device=DEV, path_length0=6)
    if demos:
        demo = golden("trace.npz")["demo_set"]
        G = n // EPG
        pts = np.concatenate([demo + 0.5 * k for k in range(G)])
        env.set_demo(pts, np.arange(G + 1, dtype=np.int64) * len(demo))
    return env


def snapshot(env):
    return {k: getattr(env, k).clone() for k in SOA}


def restore(env, snap):
    for k in SOA:
        getattr(env, k).copy_(snap[k])


def member_view(name, t, m, epm=EPM):
    """Member m's part of a per-env tensor (hist is [5][n][2], block_stats [n / 64][8])."""
    if name == "hist":
        return t[:, m * epm:(m + 1) * epm]
    if name == "block_stats":
        return t[m * epm // 64:(m + 1) * epm // 64]
    return t[m * epm:(m + 1) * epm]


def run_ticks(env, ticks, tick_fn):
    """`ticks` launches of tick_fn(t, action, reward); per tick the step outputs, the actions and
    the rewards of the flagged envs (the buffer is zeroed before every launch)."""
    action = torch.zeros(env.n, 2, dtype=torch.float64, device=DEV)
    reward = torch.zeros(env.n, dtype=torch.float64, device=DEV)
    rec = []
    for t in range(ticks):
        reward.zero_()
        extra = tick_fn(t, action, reward)
        r = {k: getattr(env, k).clone() for k in STEP_OUT}
        r["action"], r["reward"] = action.clone(), reward.clone()
        r.update(extra or {})
        rec.append(r)
    return rec


_tick_cases = {}


def tick_case(hidden, demos):
    """The distinct-member population run and the three single-policy runs, once per shape."""
    key = (hidden, demos)
    if key in _tick_cases:
        return _tick_cases[key]
    from nav.population import PopulationTable
    from nav.vec_env import ReplayRing
    env = make_env(N, demos)
    start = snapshot(env)
    actors = [make_actor(hidden, 2, 31 + m)[0] for m in range(P)]
    params = [member_params(m) for m in range(P)]
    cap = P * EPM  # 3 ticks of a member: the rings wrap 13 times in 40 ticks
    ring_rows = torch.zeros(P, cap, 8, dtype=torch.float32, device=DEV)
    rings = [ReplayRing(cap, DEV, rows=ring_rows[m]) for m in range(P)]
    pop = PopulationTable(actors, params, rings, EPM)

    def pop_tick(t, action, reward):
        base = rings[0].position
        env.act_tick_pop(pop, t, base, action_out=action, reward_out=reward)
        for r in rings:
            r.advance(EPM)
        slots = (base + torch.arange(EPM, device=DEV)) % cap
        return {"rows": ring_rows[:, slots].clone()}  # [P][EPM][8]: the rows just written

    got = run_ticks(env, TICKS, pop_tick)
    got_end = snapshot(env)
    refs = []
    for m in range(P):
        restore(env, start)
        env.p = params[m]
        ring = ReplayRing(TICKS * N, DEV)  # holds every tick: tick t's env e at row t * N + e

        def ref_tick(t, action, reward):
            env.act_tick(actors[m], t, ring, action_out=action, reward_out=reward)

        rec = run_ticks(env, TICKS, ref_tick)
        refs.append((rec, snapshot(env), ring.rows.view(TICKS, N, 8).clone()))
    torch.cuda.synchronize()
    _tick_cases[key] = dict(got=got, got_end=got_end, refs=refs)
    return _tick_cases[key]


@pytest.mark.parametrize("demos", [True, False], ids=["demos", "nodemos"])
@pytest.mark.parametrize("hidden", [64, 256, 24, 150])
def test_tick_distinct_members(nav, hidden, demos):
    """P = 3 x 128 envs, members differing in actor weights, demo_factor, noise_decay,
    stuck_penalty, goal_reward and path_increase, 40 ticks from a common start, rings of 3 x 128
    rows (they wrap): the nine SoA arrays, next_state, goal_term, flags, action_out, reward_out,
    every ring row and the block_stats rows of member m equal the single-policy run with actor m
    and params m on member m's slice."""
    c = tick_case(hidden, demos)
    ended = 0
    for m in range(P):
        rec, end, rows = c["refs"][m]
        for t in range(TICKS):
            g, r = c["got"][t], rec[t]
            for k in STEP_OUT + ("action", "reward"):
                assert torch.equal(member_view(k, g[k], m), member_view(k, r[k], m)), (k, t, m)
            assert torch.equal(g["rows"][m], rows[t, m * EPM:(m + 1) * EPM]), ("rows", t, m)
            ended += int((member_view("flags", g["flags"], m) & 8).ne(0).sum())
        for k in SOA:
            assert torch.equal(member_view(k, c["got_end"][k], m), member_view(k, end[k], m)), k
    # conditions on the inputs: episodes ended and reset inside the run, the members' runs differ
    # (so a member served with another's actor or constants would show), demo rewards were formed
    assert ended > P * EPM
    a0, a1 = c["refs"][0][1], c["refs"][1][1]
    assert not torch.equal(a0["state"], a1["state"])
    assert not torch.equal(a0["noise_scale"], a1["noise_scale"])
    assert not torch.equal(a0["path_length"], a1["path_length"])
    if demos:
        assert sum(int((g["reward"] != 0).sum()) for g in c["got"]) > 0


def test_tick_identical_members(nav):
    """P = 3 with the same actor and params: one plain nav_act_tick over the 384 envs (the plain
    ring's slot of env e at tick t holds member e / 128's row of its local env)."""
    from nav.population import PopulationTable
    from nav.vec_env import ReplayRing
    ticks = 10
    env = make_env(N, True)
    start = snapshot(env)
    actor = make_actor(64, 2, 31)[0]
    p = member_params(0, distinct=False)
    cap = P * EPM
    ring_rows = torch.zeros(P, cap, 8, dtype=torch.float32, device=DEV)
    rings = [ReplayRing(cap, DEV, rows=ring_rows[m]) for m in range(P)]
    pop = PopulationTable([actor] * P, [p] * P, rings, EPM)

    def pop_tick(t, action, reward):
        base = rings[0].position
        env.act_tick_pop(pop, t, base, action_out=action, reward_out=reward)
        for r in rings:
            r.advance(EPM)
        slots = (base + torch.arange(EPM, device=DEV)) % cap
        return {"rows": ring_rows[:, slots].clone()}

    got = run_ticks(env, ticks, pop_tick)
    got_end = snapshot(env)
    restore(env, start)
    env.p = p
    ring = ReplayRing(ticks * N, DEV)

    def ref_tick(t, action, reward):
        env.act_tick(actor, t, ring, action_out=action, reward_out=reward)

    ref = run_ticks(env, ticks, ref_tick)
    rows = ring.rows.view(ticks, P, EPM, 8)
    for t in range(ticks):
        for k in STEP_OUT + ("action", "reward"):
            assert torch.equal(got[t][k], ref[t][k]), (k, t)
        assert torch.equal(got[t]["rows"], rows[t]), ("rows", t)
    end = snapshot(env)
    for k in SOA:
        assert torch.equal(got_end[k], end[k]), k


def test_tick_table_past_one_chunk(nav):
    """P = 7 x 64 envs at hidden 32 x 1: the smallest population whose table (7 entries of 296 B)
    spans two of the table writer's 2 KB chunks, the second one partial and member 6's entry
    across the boundary. Distinct actors and constants, 8 ticks with demos, rings of 3 x 64 rows:
    as test_tick_distinct_members, member m's slice of every output and its ring rows equal the
    single-policy run with actor m and params m."""
    from nav.population import PopulationTable
    from nav.vec_env import ReplayRing
    P7, epm, ticks = 7, 64, 8
    n = P7 * epm
    env = make_env(n, True)
    start = snapshot(env)
    actors = [make_actor(32, 1, 31 + m)[0] for m in range(P7)]
    params = [member_params(m % 3, demo_factor=10.0 + 5.0 * m) for m in range(P7)]
    cap = 3 * epm
    ring_rows = torch.zeros(P7, cap, 8, dtype=torch.float32, device=DEV)
    rings = [ReplayRing(cap, DEV, rows=ring_rows[m]) for m in range(P7)]
    pop = PopulationTable(actors, params, rings, epm)
    assert pop.table.numel() > 2048 and pop.table.numel() % 2048 != 0

    def pop_tick(t, action, reward):
        base = rings[0].position
        env.act_tick_pop(pop, t, base, action_out=action, reward_out=reward)
        for r in rings:
            r.advance(epm)
        slots = (base + torch.arange(epm, device=DEV)) % cap
        return {"rows": ring_rows[:, slots].clone()}

    got = run_ticks(env, ticks, pop_tick)
    got_end = snapshot(env)
    ends = []
    for m in range(P7):
        restore(env, start)
        env.p = params[m]
        ring = ReplayRing(ticks * n, DEV)

        def ref_tick(t, action, reward):
            env.act_tick(actors[m], t, ring, action_out=action, reward_out=reward)

        rec = run_ticks(env, ticks, ref_tick)
        rows = ring.rows.view(ticks, n, 8)
        for t in range(ticks):
            for k in STEP_OUT + ("action", "reward"):
                assert torch.equal(member_view(k, got[t][k], m, epm),
                                   member_view(k, rec[t][k], m, epm)), (k, t, m)
            assert torch.equal(got[t]["rows"][m], rows[t, m * epm:(m + 1) * epm]), ("rows", t, m)
        end = snapshot(env)
        for k in SOA:
            assert torch.equal(member_view(k, got_end[k], m, epm),
                               member_view(k, end[k], m, epm)), (k, m)
        ends.append(end)
    # a condition on the inputs: the members' runs differ, the last one's too
    assert not torch.equal(ends[0]["state"], ends[6]["state"])
    assert not torch.equal(ends[5]["state"], ends[6]["state"])


_test_cases = {}


def rollout_case(hidden, epm):
    """The population's test episodes (given starts, drawn starts) and the per-actor
    nav_test_rollout runs over the whole env set, once per shape."""
    key = (hidden, epm)
    if key in _test_cases:
        return _test_cases[key]
    from nav.population import PopulationTable
    env = make_env(P * epm, False)
    actors = [make_actor(hidden, 2, 31 + m)[0] for m in range(P)]
    params = [member_params(m, goal_threshold=2.0 + 4.0 * m, max_action=5.0 - m)
              for m in range(P)]
    pop = PopulationTable(actors, params, None, epm)
    start = random_starts(env, 9)
    got = {"given": clone_out(env.test_rollout_pop(pop, T_TEST, start=start, traj=True)),
           "drawn": clone_out(env.test_rollout_pop(pop, T_TEST, episode=2, traj=True))}
    refs = []
    for m in range(P):
        env.p = params[m]
        refs.append({"given": clone_out(env.test_rollout(actors[m], T_TEST, start=start,
                                                         traj=True)),
                     "drawn": clone_out(env.test_rollout(actors[m], T_TEST, episode=2,
                                                         traj=True))})
    torch.cuda.synchronize()
    _test_cases[key] = dict(got=got, refs=refs, epm=epm)
    return _test_cases[key]


# 128: 32-row workgroups (n <= 16384); 5504 = 86 * 64: n = 16512, the 64-row side of the switch
@pytest.mark.parametrize("epm", [EPM, 5504])
@pytest.mark.parametrize("hidden", [64, 256, 24, 150])
def test_test_rollout(nav, hidden, epm):
    """Per-member actor, goal_threshold and max_action, given and drawn starts, traj, 12 steps:
    member m's slice of every output equals nav_test_rollout with actor m and params m."""
    c = rollout_case(hidden, epm)
    for form in ("given", "drawn"):
        got = c["got"][form]
        for m in range(P):
            ref = c["refs"][m][form]
            sl = slice(m * epm, (m + 1) * epm)
            for k in ("reached", "steps", "best_distance", "final_state"):
                assert torch.equal(got[k][sl], ref[k][sl]), (form, k, m)
            assert torch.equal(got["traj"][:, sl], ref["traj"][:, sl]), (form, m)
    # conditions on the inputs: rows that stop at step 1 beside rows that run on, and members
    # whose thresholds matter (member 2 reaches where member 0 does not)
    g = c["got"]["given"]
    assert int((g["steps"] == 1).sum()) > 0 and int((g["reached"] == 0).sum()) > 0
    r0, r2 = c["refs"][0]["given"]["reached"], c["refs"][2]["given"]["reached"]
    assert not torch.equal(r0, r2)


TRAINER = dict(hidden=64, n_hidden=2, batch=128, updates_per_step=2, seed=1234,
               envs_per_group=128)


def test_trainer_one_member_is_vectrainer(nav):
    """PopulationTrainer with P = 1 after 6 steps at n = 256, batch 128, hidden 64 equals
    VecTrainer with the same arguments: env state, ring, every parameter and Adam moment."""
    from nav.population import PopulationTrainer
    from nav.trainer import VecTrainer
    pt = PopulationTrainer([{}], envs_per_member=256, device=DEV, **TRAINER)
    vt = VecTrainer(n_envs=256, device=DEV, **TRAINER)
    for _ in range(6):
        pt.step()
        vt.step()
    torch.cuda.synchronize()
    sd = vt.state_dict()
    want = {"env": sd["env"], "replay": sd["replay"], "td3": sd["td3"],
            "steps": sd["meta"]["steps"]}
    _equal_tree(member_state(pt, 0), want)
    assert pt.td3[0].update_counter == 12  # a condition: the learner ran on every step


def test_trainer_isolation_and_streams(nav):
    """P = 2: changing only member 1's demo_factor and critic_lr leaves member 0's env slice,
    ring and parameters bit-identical (and changes member 1's); streams=1 and streams=4 give
    identical everything."""
    from nav.population import PopulationTrainer

    def run(members, streams):
        tr = PopulationTrainer(members, envs_per_member=256, streams=streams, device=DEV,
                               **TRAINER)
        for _ in range(6):
            tr.step()
        torch.cuda.synchronize()
        return [member_state(tr, m) for m in range(2)]

    changed = [{}, {"demo_factor": 30.0, "critic_lr": 1e-4}]
    a = run([{}, {}], 1)
    b = run(changed, 1)
    b4 = run(changed, 4)
    _equal_tree(a[0], b[0])
    assert not torch.equal(a[1]["replay"]["rows"], b[1]["replay"]["rows"])  # demo_factor
    assert not torch.equal(a[1]["td3"]["critic1"]["params"], b[1]["td3"]["critic1"]["params"])
    _equal_tree(b, b4)


def test_evaluate(nav):
    """evaluate()'s per-member numbers equal torch reductions over member m's slice of the
    single-policy nav_test_rollout with member m's actor and constants, and carry the member's
    overrides; the training state is untouched."""
    from nav.population import PopulationTrainer
    members = [{"goal_threshold": 2.0 + 4.0 * m, "seed": 5 + m} for m in range(P)]
    tr = PopulationTrainer(members, envs_per_member=EPM, demos=False, device=DEV, **TRAINER)
    tr.step()
    before = [member_state(tr, m) for m in range(P)]
    start = random_starts(tr.env, 9)
    res = tr.evaluate(max_steps=T_TEST, episode=2, start=start)
    torch.cuda.synchronize()
    _equal_tree([member_state(tr, m) for m in range(P)], before)
    keys = {"n", "success_rate", "mean_steps_reached", "mean_best_distance",
            "max_best_distance", "max_steps", "episode"}
    rates = []
    for m in range(P):
        tr.env.p = tr.params[m]
        out = tr.env.test_rollout(tr.td3[m].actor_network, T_TEST, episode=2, start=start)
        sl = tr.member_slice(m)
        reached = out["reached"][sl].bool()
        assert int(reached.sum()) > 0
        want = {"n": EPM, "success_rate": out["reached"][sl].float().mean().item(),
                "mean_steps_reached": out["steps"][sl][reached].double().mean().item(),
                "mean_best_distance": out["best_distance"][sl].mean().item(),
                "max_best_distance": out["best_distance"][sl].max().item(),
                "max_steps": T_TEST, "episode": 2}
        want.update(members[m])
        assert set(res[m]) == keys | set(members[m])
        assert res[m] == want, m
        rates.append(want["success_rate"])
    assert rates[0] < rates[2]  # a condition: the members' thresholds matter
