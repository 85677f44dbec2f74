"""Pin the oracle's goal-reached, path-end, stuck-coincidence, test-episode and demonstration-push
paths to vectors the reference itself produced (tests/golden/make_golden.py: trace_branches.npz,
test_episodes.npz, and the demo ticks of trace.npz that no test read before). CPU only.

trace.npz never reaches the goal and never ends an episode by its length, so before these
fixtures the oracle's `goal_reached`, `done` and their coincidences with `stuck` were only ever
compared with the kernels written from the same reading of robot.py. The helpers
(tests/trace_support.py) are shared with the GPU tests, which hold the kernels to the same files."""
import numpy as np
import pytest

from conftest import golden
from trace_support import (BRANCH_TRACES, DEMO_CASES, TRACES, assert_demo_rows, branch_counts,
                           carried_first_stuck, check_goal_row, demo_cases, episode_slices,
                           init_mirror, step_ticks, want_flags)


# ---- the fixtures still hold what they were made to hold ----
@pytest.mark.parametrize("name", BRANCH_TRACES)
def test_trace_branches_fixture_conditions(name):
    """A regeneration of the scripted traces cannot quietly lose a branch: the counts they were
    made for, asserted on the committed files. trace_branches.npz (constant field) carries every
    branch and coincidence; trace_branches_field.npz (a make_fields field, steering home through
    it) adds goal, path-end and stuck steps under varying dynamics and demonstration terms."""
    t = golden(name)
    n = branch_counts(t)
    print("trace.npz", branch_counts(golden("trace.npz")))
    print(name, n)
    assert n["step"] <= 800 and n["demo"] == 3
    if name == "trace_branches.npz":
        assert n["goal"] >= 8 and n["done"] >= 6 and n["stuck"] >= 6
        assert len(n["done_path_lengths"]) >= 3
        assert n["goal_stuck"] >= 1 and n["goal_done"] >= 1 and n["done_stuck"] >= 1
        # blocked: env.step returned the unchanged state object (environment.py:125 false).
        # After the clip of environment.py:117 only a NaN action can do that; pushing into a
        # world edge is clipped instead, and counted separately
        assert n["blocked"] >= 5 and n["clipped"] >= 5
        assert len(carried_first_stuck(t)) >= 2
    else:
        assert n["goal"] >= 5 and n["done"] >= 2 and n["stuck"] >= 3 and n["blocked"] >= 5
        assert len(np.unique(t["speed"])) > 1000  # not the constant field
    # no threshold within a last-bit difference of a recorded value
    first, ticks = step_ticks(t)
    hist = []
    for i in range(len(t["tick_type"])):  # robot.py:509-538, to find every compared difference
        if t["tick_type"][i] != 0:
            continue
        s = t["tick_state"][i]
        assert abs(np.linalg.norm(t["tick_next"][i] - t["goal"]) - 5.0) > 1e-6, i
        if len(hist) >= 5:
            d = [np.linalg.norm(s - q) for q in hist[-5:]]
            assert min(abs(x - 2.0) for x in d) > 1e-6, i
            stuck = all(x < 2.0 for x in d)
            assert stuck == (t["step_stuck"][i] == 1), i
            hist = [] if stuck else hist[1:]
        else:
            assert t["step_stuck"][i] == 0
        hist.append(s)
    assert ticks[0][0] == first and len(ticks) == n["step"]
    # every episode end is followed by the reference's reset tick (the file ends on one)
    assert t["tick_type"][-1] == 2
    import os
    from conftest import GOLDEN
    for f in BRANCH_TRACES + ("test_episodes.npz",):
        assert os.path.getsize(os.path.join(GOLDEN, f)) <= 317006


def test_test_episodes_fixture_conditions():
    g = golden("test_episodes.npz")
    for p, margin in (("a_", 1e-3), ("b_", 1e-6)):
        rs = g[p + "reached_step"]
        print(p, "pairs", len(g[p + "ep"]), "reached", int((rs > 0).sum()), "unreached",
              int((rs < 0).sum()), "clipped", int(g[p + "clipped"].sum()))
        assert np.abs(g[p + "dist"] - 5.0).min() > margin
        for e, ix in enumerate(episode_slices(g, p)):
            d = g[p + "dist"][ix]
            hit = np.nonzero(d <= 5.0)[0]
            assert rs[e] == (hit[0] + 1 if len(hit) else -1)
            assert len(ix) == (rs[e] if rs[e] > 0 else int(g[p + "cap"]))
            # consecutive steps chain, the first one starts at the chosen start
            assert np.array_equal(g[p + "state"][ix][0], g[p + "start"][e])
            assert np.array_equal(g[p + "state"][ix][1:], g[p + "next"][ix][:-1])
    ra, rb6 = g["a_reached_step"], g["b6_reached_step"]
    assert (ra > 0).sum() >= 5 and (ra < 0).sum() >= 5
    assert (rb6 > 0).sum() >= 5 and (rb6 < 0).sum() >= 5  # group (b) under the cap of 6
    assert (g["b_reached_step"] > 0).all()
    assert g["b_reached_step"].min() == 1 and g["b_reached_step"].max() >= 15
    assert np.array_equal(rb6, np.where(g["b_reached_step"] <= 6, g["b_reached_step"], -1))
    assert len(g["a_ep"]) % 64 != 0  # the GPU test's last tile is partial
    # blocked as the reference defines it (the unchanged state object) cannot happen in testing
    # mode: the actor's clipped action is never NaN. Steps clipped at a world edge stand in
    assert g["a_blocked"].sum() == 0 and g["b_blocked"].sum() == 0
    assert g["a_clipped"].sum() >= 3


# ---- the training tick ----
def _replay_tick(orc, t, tick):
    """Replay a trace through `tick(st, action, reset_state) -> (flags, ns, row, r)` with
    test_agent_trace_vs_reference's assertions and bounds; returns the per-step flags."""
    first, ticks = step_ticks(t)
    st = init_mirror(orc, t, first)
    c = t["counters"]
    flags_seen = []
    for i, lo, reset_state in ticks:
        flags, ns, row, r = tick(st, t["tick_action"][i], reset_state)
        assert np.max(np.abs(ns - t["push_s2"][lo])) < 1e-12, i
        assert abs(r - t["push_r"][lo]) <= 1e-9 * max(1.0, abs(t["push_r"][lo])), i
        assert bool(flags & 1) == bool(t["push_d"][lo]), i
        assert row[4] == np.float32(t["push_r"][lo]), i
        assert row[7] == float(t["push_d"][lo]), i
        assert np.array_equal(row[[0, 1, 5, 6]],
                              np.concatenate([t["push_s"][lo], t["push_s2"][lo]]).astype(
                                  np.float32)), i
        assert np.array_equal(row[2:4], t["push_a"][lo].astype(np.float32), equal_nan=True), i
        if reset_state is not None:
            cc = c[i + 1]
            assert st.episodes[0] == int(cc[2]) and st.path_length[0] == int(cc[1])
            assert st.noise_scale[0] == cc[6]
            assert st.plan_index[0] == 1 and int(cc[0]) == 0
            st.state[0] = reset_state  # (the batched forms draw their own: overwrite it)
        else:
            assert (st.meta[0] & 3) == 0
            assert st.plan_index[0] == int(c[i][0]) + 1
        if "step_goal" in t.files:
            assert (flags & 15) == want_flags(t, i, lo, reset_state), (i, flags)
            check_goal_row(t, i, lo, row[4])
            assert r == t["push_r"][lo] or t["step_goal"][i] == 0
        flags_seen.append(flags & 15)
    return np.array(flags_seen)


@pytest.mark.parametrize("name", BRANCH_TRACES)
def test_agent_tick_vs_reference_branches(orc, name):
    """The scripted traces through the oracle's fused tick with the reference's actions and reset
    states: test_agent_trace_vs_reference's checks, plus every flag bit against the reference's
    own record (done = push_d, goal_reached and stuck_flag right after process_transition,
    ended = its next tick is a reset), the pushed state / action / next-state columns, and the
    goal rows' rewards exactly (50, or 0 when stuck on the same step)."""
    t = golden(name)
    p = orc.default_params()

    def tick(st, a, reset_state):
        return st.tick(p, t["speed"], t["angle"], t["demo_set"], 0, a, reset_state)

    fl = _replay_tick(orc, t, tick)
    n = branch_counts(t)
    assert int((fl & 2 > 0).sum()) == n["goal"] and int((fl & 1).sum()) == n["done"]
    assert int((fl & 4 > 0).sum()) == n["stuck"] and int((fl & 8 > 0).sum()) == n["reset"] - 1


@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("name", TRACES)
def test_step_batch_replays_reference_trace(orc, name, indexed):
    """Both reference traces through VecAgentState.step_batch (the entry point the GPU tests
    compare whole launches with), brute-force and through the exact demo index: the same checks
    as the per-env tick. step_batch draws its own reset state, so the reference's is written
    over it after every ended step."""
    t = golden(name)
    p = orc.default_params()
    demo = np.ascontiguousarray(t["demo_set"])
    index = orc.DemoIndexCPU(demo) if indexed else None
    rows = np.zeros((7, 8), np.float32)
    base = [0]

    def tick(st, a, reset_state):
        ns, fl, r = st.step_batch(p, t["speed"], t["angle"], demo, a[None], rows, base[0],
                                  index=index)
        row = rows[base[0] % 7].copy()
        base[0] += 1
        assert bool(fl[0] & 8) == (reset_state is not None)
        return int(fl[0]), ns[0], row, float(r[0])

    _replay_tick(orc, t, tick)


# ---- the testing mode ----
def test_test_episodes_vs_reference(orc):
    """Every recorded step of the reference's testing loop (robot-learning.py:104-117): the action
    epilogue bit for bit from the recorded residual, the env step and the distance within 1e-12
    (atan2 may differ by an ulp), the reached step and best distance recomputed the reference's
    way (`<=` after each step, never at the start state; best tracked with `<` after the threshold
    test) equal to the fixture's, and the torch-CPU forward of the fixture's actor within the
    residual bound of test_action_epilogue_and_actor_vs_reference."""
    import torch
    from oracle.td3_oracle import MLP, make_mlp_params
    g = golden("test_episodes.npz")
    actor = MLP(make_mlp_params(int(g["a_actor_seed"]), [2, 200, 200, 200, 2]))
    ga = g["a_goal"][g["a_ep"]]
    with torch.no_grad():
        res = actor.forward(torch.tensor((g["a_state"] - ga).astype(np.float32))).numpy()
    assert np.allclose(res, g["a_residual"], rtol=2e-5, atol=1e-4)
    fields = {"a_": (g["a_speed"], g["a_angle"]),
              "b_": (np.full((100, 100), 1.0, np.float32), np.full((100, 100), 0.5, np.float32))}
    for p in ("a_", "b_"):
        sp, an = fields[p]
        for e, ix in enumerate(episode_slices(g, p)):
            goal = g[p + "goal"][e]
            best, reached = np.inf, -1
            for k in ix:
                s = g[p + "state"][k]
                a = orc.act_epilogue(s, goal, g[p + "residual"][k], 0, None)
                assert np.array_equal(a, g[p + "action"][k]), (p, e)
                ns, ok = orc.step(sp, an, s, a)
                assert ok == 1 and np.max(np.abs(ns - g[p + "next"][k])) < 1e-12, (p, e)
                d = orc.norm2(ns[0] - goal[0], ns[1] - goal[1])
                assert abs(d - g[p + "dist"][k]) < 1e-12
                if d <= 5.0:
                    reached = int(g[p + "t"][k]) + 1
                    break
                if d < best:
                    best = d
            assert reached == g[p + "reached_step"][e], (p, e)
            want = g[p + "best"][e]
            assert best == want or abs(best - want) < 1e-12, (p, e)
            if reached == 1:
                assert np.isinf(want)  # the reaching step never updates the best distance
    # the cap of 6 cuts group (b)'s longer episodes off: the same loop, stopped earlier
    for e, ix in enumerate(episode_slices(g, "b_")):
        d = g["b_dist"][ix][:6]
        hit = len(ix) <= 6
        assert g["b6_steps"][e] == min(len(ix), 6)
        assert np.array_equal(g["b6_final"][e], g["b_next"][ix][min(len(ix), 6) - 1])
        assert g["b6_best"][e] == (d[:-1].min() if hit and len(d) > 1 else
                                   np.inf if hit else d.min())


# ---- the demonstration pushes ----
@pytest.mark.parametrize("case", range(4), ids=DEMO_CASES)
def test_demo_transitions_ref_vs_reference_pushes(case):
    """nav_demo_transitions' numpy restatement (frame 0) on the demonstrations the reference drew
    against what its process_demonstration pushed (robot.py:704-716): the reward it formed with
    demonstration_states already extended and demo_flag false is the goal term alone, the done
    row is the last one. One of trace_branches.npz's CEM demonstrations ends inside the goal
    radius (its done row carries the goal reward); the hand-made path does so by construction."""
    from nav.demo_replay import transitions_ref
    name, st, ac, goals, want, rew = demo_cases()[case]
    got = transitions_ref(st, ac, goals, 0)
    n_goal, n_ulp = assert_demo_rows(got, want, rew)
    print(f"{name}: {len(got)} rows, {n_goal} inside the goal radius, {n_ulp} rewards one ulp off")
    T = st.shape[1]
    assert got[:, 7].sum() == len(st) and (got[T - 2::T - 1, 7] == 1).all()
    if name == "hand":
        assert n_goal >= 2 and rew[-1] == 50.0 and (rew < -5.0).any()
