"""The environment, demo-reward, demo-index and demonstrator entry points, host side: every case
below returns either the raw status NAV_EINVAL or 0 before any HIP call (no kernel is launched,
the dummy pointers are never followed, so no GPU is needed). One case per clause of each entry
point's argument check, and the zero-size returns with the pointers null that are looked at only
after them (the order of the checks). Recorded from the library before env_kernels.hip was split
by subject; the learner entry points' table is tests/test_learner_args_cpu.py."""
import ctypes as C

import pytest

from abi_args import EINVAL, F, Call, load_raw, v

ENV_PTRS = ("state", "goal", "region", "hist", "meta", "plan_index", "path_length", "episodes",
            "noise_scale")


@pytest.fixture(scope="module")
def raw():
    return load_raw()


def params(**kw):
    from nav._lib import NavParams
    kw.setdefault("max_goal_draws", 1 << 16)
    return lambda: C.byref(NavParams(**kw))


def env(n=65, **fields):
    """nav_env_soa of n envs, every array a dummy pointer but the ones named (None = NULL)"""
    from nav._lib import NavEnvSoa
    return lambda: C.byref(NavEnvSoa(n, *[fields.get(k, F) for k in ENV_PTRS]))


EMPTY_ENV = env(0, **{k: None for k in ENV_PTRS})


def replay(rows=F, capacity=128):
    from nav._lib import NavReplay
    return lambda: C.byref(NavReplay(rows, capacity))


def step_out():
    from nav._lib import NavStepOut
    return C.byref(NavStepOut())


_P, _S = dict(p=params()), dict(stream=v(None))
_RING = dict(replay=replay(), replay_base=v(3))
_IDX = dict(demo_xy=v(F), demo_off=v(F), envs_per_group=v(13), cell_start=v(F), cand=v(F))
_GROUPS = dict(demo_xy=v(F), demo_off=v(F), n_groups=v(2))

CALLS = {c.fn: c for c in (
    Call("nav_env_init", **_P, env=env(), envs_per_group=v(13), demo_flag=v(0),
         draws_out=v(None), **_S),
    Call("nav_env_reset", **_P, env=env(), mask=v(None), uniforms=v(None), **_S),
    Call("nav_env_step", **_P, env=env(), field=v(F), action=v(F), next_state=v(None), **_S),
    Call("nav_env_step_k", **_P, env=env(), field=v(F), actions=v(F), K=v(3), next_states=v(None),
         **_S),
    Call("nav_dynamics", field=v(F), state=v(F), action=v(F), out=v(F), n=v(65), **_S),
    Call("nav_agent_step", **_P, env=env(), field=v(F), action=v(F), **_RING, out=step_out,
         demo_pending=v(0), **_S),
    Call("nav_agent_step_indexed", **_P, env=env(), field=v(F), action=v(F), **_RING,
         out=step_out, **_IDX, reward_out=v(None), **_S),
    Call("nav_transition", **_P, env=env(), state=v(F), action=v(F), next_state=v(F), **_RING,
         out=step_out, demo_pending=v(0), **_S),
    Call("nav_check_if_stuck", **_P, env=env(), state=v(F), stuck=v(F), **_S),
    Call("nav_compute_reward", **_P, n=v(65), next_state=v(F), goal=v(F), demo_xy=v(F), m=v(7),
         demo_flag=v(1), reward=v(F), goal_hit=v(None), **_S),
    Call("nav_replay_push", replay=replay(), base=v(3), n=v(65), state=v(F), action=v(F),
         reward=v(F), next_state=v(F), done=v(F), **_S),
    Call("nav_demo_reward", **_P, n=v(65), next_state=v(F), goal_term=v(F), flags=v(F),
         demo_xy=v(F), demo_off=v(F), m=v(0), envs_per_group=v(13), **_RING, reward_out=v(None),
         block_stats=v(None), **_S),
    Call("nav_demo_reward_indexed", **_P, n=v(65), next_state=v(F), goal_term=v(F), flags=v(F),
         **_IDX, **_RING, reward_out=v(None), block_stats=v(None), **_S),
    Call("nav_demo_min", points=v(F), n=v(65), demo_xy=v(F), m=v(7), out=v(F), **_S),
    Call("nav_demo_index_plan", **_GROUPS, m=v(0), cell_bound=v(F), cell_count=v(F), **_S),
    Call("nav_demo_index_scan", cell_count=v(F), n_groups=v(2), cell_start=v(F), **_S),
    Call("nav_demo_index_fill", **_GROUPS, m=v(0), cell_bound=v(F), cell_start=v(F), cand=v(F),
         **_S),
    Call("nav_demo_index_subplan", **_GROUPS, cell_start=v(F), cand=v(F), sub_bound=v(F),
         sub_count=v(F), **_S),
    Call("nav_demo_index_subscan", sub_count=v(F), n_groups=v(2), sub_start=v(F), **_S),
    Call("nav_demo_index_subfill", **_GROUPS, cell_start=v(F), cand=v(F), sub_bound=v(F),
         sub_start=v(F), sub_cand=v(F), **_S),
    Call("nav_rollout", field=v(F), P=v(65), T=v(4), start=v(F), actions=v(F), paths=v(F),
         goal=v(F), reward=v(F), **_S),
    Call("nav_cem_rollout", field=v(F), n_prob=v(3), P=v(40), T=v(5), iter=v(0), region=v(F),
         uniforms=v(F), goal=v(F), a0=v(F), z=v(F), mean=v(F), stdv=v(F), actions=v(F),
         paths=v(None), reward=v(F), **_S),
    Call("nav_cem_elite", n_prob=v(3), P=v(40), T=v(5), E=v(8), reward=v(F), actions=v(F),
         mean=v(F), stdv=v(F), best=v(None), **_S),
    Call("nav_fields_generate", g5=v(F), g10=v(F), g20=v(F), field=v(F), **_S),
    Call("nav_demo_augment", n_demo=v(3), T=v(5), steps=v(2), n_aug=v(2), states=v(F),
         noise=v(F), out=v(F), **_S),
    Call("nav_event_create", event=v(None)),
    Call("nav_event_destroy", event=v(None)),
    Call("nav_event_record", event=v(None), stream=v(None)),
    Call("nav_event_elapsed_ms", start=v(F), end=v(F), ms=lambda: C.byref(C.c_float())),
)}


def nulls(fn, *names):
    return [(fn, f"no {k}", {k: v(None)}) for k in names]


def env_nulls(fn, *fields):
    return [(fn, f"no env.{k}", dict(env=env(**{k: None}))) for k in fields]


def ring(fn, slot_per_env, base="replay_base"):
    """The replay-ring guard's clauses; slot_per_env: the ring must hold one slot per env"""
    out = nulls(fn, "replay") + [
        (fn, "no replay.rows", dict(replay=replay(rows=None))),
        (fn, "capacity = 0", dict(replay=replay(capacity=0))),
        (fn, f"{base} < 0", {base: v(-1)}),
    ]
    if slot_per_env:
        out.append((fn, "capacity < n", dict(replay=replay(capacity=64))))
    return out


def groups(fn):
    """The demo set of the index builders: per-group offsets, or one shared group"""
    return nulls(fn, "demo_xy") + [
        (fn, "n_groups = 0", dict(n_groups=v(0))),
        (fn, "shared demos, n_groups = 2", dict(demo_off=v(None))),
    ]


ALL_NULL_IDX = {k: v(None) for k in ("demo_xy", "cell_start", "cand")}

# (entry point, what is wrong, the altered arguments)
BAD = (
    nulls("nav_env_init", "p", "env") + env_nulls("nav_env_init", *ENV_PTRS) + [
        ("nav_env_init", "n < 0", dict(env=env(-1))),
        ("nav_env_init", "n = 2^31", dict(env=env(1 << 31))),
        ("nav_env_init", "epg = 0", dict(envs_per_group=v(0))),
        ("nav_env_init", "epg = 0 and no envs", dict(envs_per_group=v(0), env=EMPTY_ENV)),
        ("nav_env_init", "max_goal_draws = 0", dict(p=params(max_goal_draws=0))),
    ] + nulls("nav_env_reset", "p", "env") + env_nulls("nav_env_reset", "state", "region") + [
        ("nav_env_reset", "n < 0", dict(env=env(-1))),
        ("nav_env_reset", "neither uniforms nor env.episodes", dict(env=env(episodes=None))),
    ] + nulls("nav_env_step", "p", "env", "field", "action")
    + env_nulls("nav_env_step", "state") + [
        ("nav_env_step", "n < 0", dict(env=env(-1))),
        ("nav_env_step", "no field and no envs", dict(field=v(None), env=EMPTY_ENV)),
    ] + nulls("nav_env_step_k", "p", "env", "field", "actions")
    + env_nulls("nav_env_step_k", "state") + [
        ("nav_env_step_k", "n < 0", dict(env=env(-1))),
        ("nav_env_step_k", "K < 0", dict(K=v(-1))),
        ("nav_env_step_k", "no field and K = 0", dict(field=v(None), K=v(0))),
    ] + nulls("nav_dynamics", "field", "state", "action", "out") + [
        ("nav_dynamics", "n < 0", dict(n=v(-1))),
    ] + nulls("nav_agent_step", "p", "env", "field", "action", "out")
    + env_nulls("nav_agent_step", *ENV_PTRS) + ring("nav_agent_step", True) + [
        ("nav_agent_step", "n < 0", dict(env=env(-1))),
        ("nav_agent_step", "n = 2^31", dict(env=env(1 << 31), replay=replay(capacity=1 << 32))),
        ("nav_agent_step", "capacity = 0 and no envs",
         dict(env=EMPTY_ENV, replay=replay(capacity=0))),
    ] + nulls("nav_agent_step_indexed", "p", "env", "field", "action", "out", "demo_xy",
              "cell_start", "cand")
    + env_nulls("nav_agent_step_indexed", "noise_scale") + ring("nav_agent_step_indexed", True) + [
        ("nav_agent_step_indexed", "demo_off and epg = 0", dict(envs_per_group=v(0))),
        ("nav_agent_step_indexed", "demo_off and epg = 0 and no envs",
         dict(envs_per_group=v(0), env=EMPTY_ENV)),
    ] + nulls("nav_transition", "p", "env", "out", "state", "action", "next_state")
    + env_nulls("nav_transition", "goal", "hist", "meta", "plan_index", "path_length")
    + ring("nav_transition", True) + [
        ("nav_transition", "n < 0", dict(env=env(-1))),
    ] + nulls("nav_check_if_stuck", "p", "env", "state", "stuck")
    + env_nulls("nav_check_if_stuck", "hist", "meta") + [
        ("nav_check_if_stuck", "n < 0", dict(env=env(-1))),
    ] + nulls("nav_compute_reward", "p", "next_state", "goal", "reward", "demo_xy") + [
        ("nav_compute_reward", "n < 0", dict(n=v(-1))),
        ("nav_compute_reward", "m < 0", dict(m=v(-1))),
        ("nav_compute_reward", "m > 0, no demo_xy and n = 0", dict(n=v(0), demo_xy=v(None))),
    ] + ring("nav_replay_push", False, "base")
    + nulls("nav_replay_push", "state", "action", "reward", "next_state", "done") + [
        ("nav_replay_push", "n < 0", dict(n=v(-1))),
    ] + nulls("nav_demo_reward", "p", "next_state", "goal_term", "flags")
    + ring("nav_demo_reward", False) + [
        ("nav_demo_reward", "n < 0", dict(n=v(-1))),
        ("nav_demo_reward", "demo_off and epg = 0", dict(envs_per_group=v(0))),
        ("nav_demo_reward", "demo_off and epg = 0 and n = 0", dict(envs_per_group=v(0), n=v(0))),
        ("nav_demo_reward", "shared demos, m > 0, no demo_xy",
         dict(demo_off=v(None), m=v(7), demo_xy=v(None))),
    ] + nulls("nav_demo_reward_indexed", "p", "next_state", "goal_term", "flags", "demo_xy",
              "cell_start", "cand")
    + ring("nav_demo_reward_indexed", False) + [
        ("nav_demo_reward_indexed", "n < 0", dict(n=v(-1))),
        ("nav_demo_reward_indexed", "demo_off and epg = 0", dict(envs_per_group=v(0))),
        ("nav_demo_reward_indexed", "demo_off and epg = 0 and n = 0",
         dict(envs_per_group=v(0), n=v(0))),
    ] + nulls("nav_demo_min", "points", "demo_xy", "out") + [
        ("nav_demo_min", "n < 0", dict(n=v(-1))),
        ("nav_demo_min", "m = 0", dict(m=v(0))),
        ("nav_demo_min", "m = 0 and n = 0", dict(m=v(0), n=v(0))),
    ] + groups("nav_demo_index_plan")
    + nulls("nav_demo_index_plan", "cell_bound", "cell_count") + [
        ("nav_demo_index_plan", "shared demos, m = 0", dict(demo_off=v(None), n_groups=v(1))),
    ] + nulls("nav_demo_index_scan", "cell_count", "cell_start") + [
        ("nav_demo_index_scan", "n_groups = 0", dict(n_groups=v(0))),
    ] + groups("nav_demo_index_fill")
    + nulls("nav_demo_index_fill", "cell_bound", "cell_start", "cand")
    + groups("nav_demo_index_subplan")
    + nulls("nav_demo_index_subplan", "cell_start", "cand", "sub_bound", "sub_count")
    + nulls("nav_demo_index_subscan", "sub_count", "sub_start") + [
        ("nav_demo_index_subscan", "n_groups = 0", dict(n_groups=v(0))),
    ] + groups("nav_demo_index_subfill")
    + nulls("nav_demo_index_subfill", "cell_start", "cand", "sub_bound", "sub_start", "sub_cand")
    + nulls("nav_rollout", "field", "start", "actions", "paths") + [
        ("nav_rollout", "P < 0", dict(P=v(-1))),
        ("nav_rollout", "T < 0", dict(T=v(-1))),
        ("nav_rollout", "reward without goal", dict(goal=v(None))),
        ("nav_rollout", "reward without goal and P = 0", dict(goal=v(None), P=v(0))),
    ] + nulls("nav_cem_rollout", "field", "region", "uniforms", "goal", "actions", "reward") + [
        ("nav_cem_rollout", "n_prob < 0", dict(n_prob=v(-1))),
        ("nav_cem_rollout", "P = 0", dict(P=v(0))),
        ("nav_cem_rollout", "T = 0", dict(T=v(0))),
        ("nav_cem_rollout", "iter < 0", dict(iter=v(-1))),
        ("nav_cem_rollout", "iter = 0 without a0", dict(a0=v(None))),
        ("nav_cem_rollout", "iter = 1 without z", dict(iter=v(1), z=v(None))),
        ("nav_cem_rollout", "iter = 1 without mean", dict(iter=v(1), mean=v(None))),
        ("nav_cem_rollout", "iter = 1 without stdv", dict(iter=v(1), stdv=v(None))),
        # 2^20 problems x 2^20 paths x (1 + 1) states = 2^41
        ("nav_cem_rollout", "over 2^40 path states",
         dict(n_prob=v(1 << 20), P=v(1 << 20), T=v(1))),
        ("nav_cem_rollout", "no field and n_prob = 0", dict(field=v(None), n_prob=v(0))),
    ] + nulls("nav_cem_elite", "reward", "actions", "mean", "stdv") + [
        ("nav_cem_elite", "n_prob < 0", dict(n_prob=v(-1))),
        ("nav_cem_elite", "P = 0", dict(P=v(0))),
        ("nav_cem_elite", "P = 257", dict(P=v(257))),
        ("nav_cem_elite", "T = 0", dict(T=v(0))),
        ("nav_cem_elite", "E = 0", dict(E=v(0))),
        ("nav_cem_elite", "E > P", dict(E=v(41))),
        ("nav_cem_elite", "E > P and n_prob = 0", dict(E=v(41), n_prob=v(0))),
    ] + nulls("nav_fields_generate", "g5", "g10", "g20", "field")
    + nulls("nav_demo_augment", "states", "noise", "out") + [
        ("nav_demo_augment", "n_demo < 0", dict(n_demo=v(-1))),
        ("nav_demo_augment", "T = 1", dict(T=v(1))),
        ("nav_demo_augment", "T = 1 and n_demo = 0", dict(T=v(1), n_demo=v(0))),
        ("nav_demo_augment", "steps < 0", dict(steps=v(-1))),
        ("nav_demo_augment", "n_aug < 0", dict(n_aug=v(-1))),
    ] + [
        ("nav_event_create", "no event", {}),
        ("nav_event_destroy", "no event", {}),
        ("nav_event_record", "no event", {}),
    ] + nulls("nav_event_elapsed_ms", "start", "end", "ms")
)

# the returns of 0 without a launch, with the pointers null that are looked at only after them
ZERO = [
    ("nav_env_init", "no envs", dict(env=EMPTY_ENV)),
    ("nav_env_reset", "no envs", dict(env=EMPTY_ENV)),
    ("nav_env_step", "no envs, no action", dict(env=EMPTY_ENV, action=v(None))),
    ("nav_env_step_k", "no envs, no actions", dict(env=EMPTY_ENV, actions=v(None))),
    ("nav_env_step_k", "K = 0, no state, no actions",
     dict(K=v(0), env=env(state=None), actions=v(None))),
    ("nav_dynamics", "n = 0, no arrays",
     dict(n=v(0), field=v(None), state=v(None), action=v(None), out=v(None))),
    ("nav_agent_step", "no envs", dict(env=EMPTY_ENV)),
    ("nav_agent_step_indexed", "no envs, no index", dict(env=EMPTY_ENV, **ALL_NULL_IDX)),
    ("nav_transition", "no envs, no state",
     dict(env=EMPTY_ENV, state=v(None), action=v(None), next_state=v(None))),
    ("nav_check_if_stuck", "no envs", dict(env=EMPTY_ENV, state=v(None), stuck=v(None))),
    ("nav_compute_reward", "n = 0, no arrays",
     dict(n=v(0), next_state=v(None), goal=v(None), reward=v(None))),
    ("nav_replay_push", "n = 0, no arrays",
     dict(n=v(0), state=v(None), action=v(None), reward=v(None), next_state=v(None),
          done=v(None))),
    ("nav_demo_reward", "n = 0, no arrays",
     dict(n=v(0), next_state=v(None), goal_term=v(None), flags=v(None))),
    ("nav_demo_reward", "shared demos, m = 0, no demo_xy",
     dict(demo_off=v(None), m=v(0), demo_xy=v(None))),
    ("nav_demo_reward_indexed", "n = 0, no next_state",
     dict(n=v(0), next_state=v(None), goal_term=v(None), flags=v(None), **ALL_NULL_IDX)),
    ("nav_demo_min", "n = 0, no arrays",
     dict(n=v(0), points=v(None), demo_xy=v(None), out=v(None))),
    ("nav_rollout", "P = 0, no arrays",
     dict(P=v(0), field=v(None), start=v(None), actions=v(None), paths=v(None))),
    ("nav_cem_rollout", "n_prob = 0", dict(n_prob=v(0))),
    ("nav_cem_elite", "n_prob = 0", dict(n_prob=v(0))),
    ("nav_demo_augment", "n_demo = 0, no arrays",
     dict(n_demo=v(0), states=v(None), noise=v(None), out=v(None))),
]


def ids(cases):
    return [f"{c[0]}-{c[1]}" for c in cases]


@pytest.mark.parametrize("fn,what,changed", BAD, ids=ids(BAD))
def test_bad_arguments_return_einval(raw, fn, what, changed):
    assert CALLS[fn](raw, **changed) == EINVAL


@pytest.mark.parametrize("fn,what,changed", ZERO, ids=ids(ZERO))
def test_nothing_to_do_returns_zero(raw, fn, what, changed):
    assert CALLS[fn](raw, **changed) == 0


def test_every_listed_entry_point_has_a_case():
    assert {b[0] for b in BAD} == set(CALLS)
    assert len(set(ids(BAD))) == len(BAD) and len(set(ids(ZERO))) == len(ZERO)


def test_default_params(raw):
    from nav._lib import NavParams
    raw.nav_default_params(None)  # ignored
    p = NavParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    raw.nav_default_params(C.byref(p))
    assert [(k, getattr(p, k)) for k, _ in NavParams._fields_] == [
        ("world_size", 100.0), ("max_action", 5.0), ("init_region_size", 25.0),
        ("goal_threshold", 5.0), ("goal_reward", 50.0), ("stuck_threshold", 2.0),
        ("stuck_penalty", 50.0), ("demo_factor", 10.0), ("noise_decay", 0.75),
        ("path_length0", 50), ("path_increase", 20), ("seed_lo", 1707366464), ("seed_hi", 0),
        ("max_goal_draws", 1 << 16)]


def test_constants(raw):
    assert raw.nav_abi_version() == 11
    assert raw.nav_demo_index_res() == 4
