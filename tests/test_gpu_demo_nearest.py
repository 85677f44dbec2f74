"""The nearest-demo index and every demo-reward launch form on ragged demo sets, against the
numpy f64 restatement tests/demo_ref.py (itself checked by test_demo_ref_cpu.py).

One layout throughout (demo_ref.ragged_layout): five groups of 1 / 3 / 70 / 11 355 / 17 points,
96 envs per group, 470 envs: the last group partial, n no multiple of 64, 64-env waves both
inside one group and across two, the first 256-env workgroup across three. Every comparison is
for equality: the kernels and the restatement do the same IEEE f64 operations in the same order
(-ffp-contract=off), and a minimum does not depend on the order it is taken in."""
import ctypes as C

import numpy as np
import pytest
import torch

import demo_ref as D
from conftest import golden
from gpu_support import nav  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -777.25   # sentinel of rows, reward_out and block_stats (exact in float32)
N, EPG = D.N_ENVS, D.EPG
F_STUCK, F_DEMO = D.F_STUCK, D.F_DEMO


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV).contiguous()


def build_index(demo_xy, demo_off, G, m):
    """The six nav_demo_index_* entry points in order (DemoIndex keeps level 2 only): both
    levels' bound, count, start and cand as device tensors."""
    from nav._lib import lib, ptr
    L = lib()
    res = int(L.nav_demo_index_res())
    c1, c2 = G * D.L1_CELLS, G * D.L1_CELLS * res * res
    out = {}
    out["bound1"] = torch.full((c1,), -1.0, dtype=torch.float64, device=DEV)
    out["count1"] = torch.full((c1,), -1, dtype=torch.int32, device=DEV)
    out["start1"] = torch.full((c1 + 1,), -1, dtype=torch.int64, device=DEV)
    L.nav_demo_index_plan(ptr(demo_xy), ptr(demo_off), G, m, ptr(out["bound1"]),
                          ptr(out["count1"]), None)
    L.nav_demo_index_scan(ptr(out["count1"]), G, ptr(out["start1"]), None)
    t1 = int(out["start1"][-1].item())
    out["cand1"] = torch.full((t1,), -1, dtype=torch.int32, device=DEV)
    L.nav_demo_index_fill(ptr(demo_xy), ptr(demo_off), G, m, ptr(out["bound1"]),
                          ptr(out["start1"]), ptr(out["cand1"]), None)
    out["bound2"] = torch.full((c2,), -1.0, dtype=torch.float64, device=DEV)
    out["count2"] = torch.full((c2,), -1, dtype=torch.int32, device=DEV)
    out["start2"] = torch.full((c2 + 1,), -1, dtype=torch.int64, device=DEV)
    L.nav_demo_index_subplan(ptr(demo_xy), ptr(demo_off), G, ptr(out["start1"]),
                             ptr(out["cand1"]), ptr(out["bound2"]), ptr(out["count2"]), None)
    L.nav_demo_index_subscan(ptr(out["count2"]), G, ptr(out["start2"]), None)
    t2 = int(out["start2"][-1].item())
    out["cand2"] = torch.full((t2,), -1, dtype=torch.int32, device=DEV)
    L.nav_demo_index_subfill(ptr(demo_xy), ptr(demo_off), G, ptr(out["start1"]),
                             ptr(out["cand1"]), ptr(out["bound2"]), ptr(out["start2"]),
                             ptr(out["cand2"]), None)
    torch.cuda.synchronize()
    return out


def layout(pts, off, s, res):
    """a layout (EPG envs per group), its query states, its index on the device, the trace's field"""
    from nav.vec_env import make_field
    t = golden("trace.npz")
    out = dict(res=res, pts=pts, off=off, s=s, n=len(s), G=len(off) - 1, demo_xy=dev(pts),
               demo_off=dev(off), field=make_field(t["speed"], t["angle"], DEV))
    assert out["G"] == (out["n"] + EPG - 1) // EPG
    out["ix"] = build_index(out["demo_xy"], out["demo_off"], out["G"], 0)
    return out


@pytest.fixture(scope="module")
def lay(nav):
    """the ragged layout"""
    from nav._lib import lib
    res = int(lib().nav_demo_index_res())
    pts, off = D.ragged_layout()
    return layout(pts, off, D.query_states(pts, off, res), res)


@pytest.fixture(scope="module")
def ring(nav):
    """the layout with long lists (demo_ref.ring_layout)"""
    from nav._lib import lib
    pts, off = D.ring_layout()
    return layout(pts, off, D.ring_states(), int(lib().nav_demo_index_res()))


def sets_of(lay):
    return [lay["pts"][lay["off"][g]:lay["off"][g + 1]] for g in range(lay["G"])]


def check_index_group(lay, ix, g, cells):
    """group g's bound, count and lists of both levels on `cells` (None: every cell, then the
    group's own scan and its whole segment of cand as well) against demo_ref"""
    res = lay["res"]
    l1, l2 = D.build(sets_of(lay)[g], res, cells)
    for lvl, ref, per in (("1", l1, D.L1_CELLS), ("2", l2, D.L1_CELLS * res * res)):
        bound, count = ix["bound" + lvl], ix["count" + lvl]
        start, cand = ix["start" + lvl][g * per:], ix["cand" + lvl]
        assert np.array_equal(bound[g * per + ref.cells], ref.bound), (g, lvl)
        assert np.array_equal(count[g * per + ref.cells], ref.count), (g, lvl)
        got_count, got = D.gather(start, cand, ref.cells)
        assert np.array_equal(got_count, ref.count), (g, lvl)
        assert np.array_equal(got, ref.cand), (g, lvl)
        if cells is None:
            assert np.array_equal(start[:per + 1] - start[0], ref.start), (g, lvl)
            assert np.array_equal(cand[start[0]:start[per]], ref.cand), (g, lvl)
    return l2


def check_scans(lay, ix):
    res = lay["res"]
    for lvl, per in (("1", D.L1_CELLS), ("2", D.L1_CELLS * res * res)):
        start, count = ix["start" + lvl], ix["count" + lvl]
        assert start[0] == 0 and np.array_equal(start[1:], np.cumsum(count, dtype=np.int64))
        assert len(ix["cand" + lvl]) == start[-1] and len(start) == lay["G"] * per + 1


# ---------------------------------------------------------------- the index build
def test_index_build_equals_reference(lay):
    """bound, count, start and cand of both levels equal demo_ref: every cell of groups A, B, C
    and E; for D 4 000 random index cells plus every cell a query state (or the tick's clip of
    it) falls in, with their level-1 parents. The scans are checked over every cell."""
    res, s = lay["res"], lay["s"]
    ix = {k: v.cpu().numpy() for k, v in lay["ix"].items()}
    c2 = D.L1_CELLS * res * res
    check_scans(lay, ix)
    rng = np.random.default_rng(42)
    mine = s[D.group_of(np.arange(N)) == 3]
    d_cells = np.unique(np.concatenate([
        rng.integers(0, c2, 4000), D.index_cell(mine, res),
        D.index_cell(np.clip(mine, 0.0, 100.0 - 1.0001), res)]))
    for g in range(5):
        check_index_group(lay, ix, g, d_cells if g == 3 else None)
    assert (ix["count2"][4 * c2:] == 17).all()
    assert (ix["count2"][:c2] == 1).all()


def test_shared_set_build_equals_one_group_build(lay):
    """demo_off = NULL with m builds what demo_off = {0, m} builds, array for array, and both
    equal group D's part of the five-group build (the lists are group-relative)."""
    res = lay["res"]
    P = sets_of(lay)[3]
    xy = dev(P)
    shared = build_index(xy, None, 1, len(P))
    one = build_index(xy, dev(np.array([0, len(P)], np.int64)), 1, 0)
    for k in shared:
        assert torch.equal(shared[k], one[k]), k
    five = lay["ix"]
    for lvl, per in (("1", D.L1_CELLS), ("2", D.L1_CELLS * res * res)):
        sl = slice(3 * per, 4 * per)
        assert torch.equal(shared["bound" + lvl], five["bound" + lvl][sl])
        assert torch.equal(shared["count" + lvl], five["count" + lvl][sl])
        a, b = int(five["start" + lvl][3 * per].item()), int(five["start" + lvl][4 * per].item())
        assert torch.equal(shared["cand" + lvl], five["cand" + lvl][a:b])


# ---------------------------------------------------------------- the reward passes alone
def written_flags(n, rng):
    """F_DEMO except on every 7th env, F_STUCK on every 5th, the other bits at random"""
    e = np.arange(n)
    fl = rng.integers(0, 16, n).astype(np.uint8) & np.uint8(0x0b)
    fl |= np.where(e % 7 != 0, F_DEMO, 0).astype(np.uint8)
    fl |= np.where(e % 5 == 0, F_STUCK, 0).astype(np.uint8)
    return fl


def reward_pass(form, lay, ns, gt, flags, epg, base=7):
    """nav_demo_reward ("brute") or nav_demo_reward_indexed ("indexed") on sentinel-filled
    outputs, into a ring of n + 3 rows from slot `base` on (the last slots wrap)"""
    from nav._lib import NavReplay, lib, params_struct, ptr, stream_handle
    n = len(ns)
    cap = n + 3
    rows = torch.full((cap, 8), SENT, dtype=torch.float32, device=DEV)
    r_out = torch.full((n,), SENT, dtype=torch.float64, device=DEV)
    stats = torch.full(((n + 63) // 64, 8), SENT, dtype=torch.float32, device=DEV)
    p = params_struct()
    rd = NavReplay(rows.data_ptr(), cap)
    a = (dev(ns), dev(gt), dev(flags))
    if form == "brute":
        lib().nav_demo_reward(C.byref(p), n, ptr(a[0]), ptr(a[1]), ptr(a[2]),
                              ptr(lay["demo_xy"]), ptr(lay["demo_off"]), 0, epg, C.byref(rd),
                              base, ptr(r_out), ptr(stats), stream_handle())
    else:
        lib().nav_demo_reward_indexed(C.byref(p), n, ptr(a[0]), ptr(a[1]), ptr(a[2]),
                                      ptr(lay["demo_xy"]), ptr(lay["demo_off"]), epg,
                                      ptr(lay["ix"]["start2"]), ptr(lay["ix"]["cand2"]),
                                      C.byref(rd), base, ptr(r_out), ptr(stats), stream_handle())
    torch.cuda.synchronize()
    return rows.cpu().numpy(), r_out.cpu().numpy(), stats.cpu().numpy()


def reward_expected(lay, ns, gt, flags, epg, base=7):
    """what reward_pass must leave: demo_ref's reward in reward_out and, as float32, in word 4 of
    the row of every flagged env; the reward column of every 64-env row holding a flagged env
    summed again from the rows; everything else still the sentinel"""
    n = len(ns)
    cap = n + 3
    sets = sets_of(lay)
    rows = np.full((cap, 8), SENT, np.float32)
    r_out = np.full(n, SENT)
    stats = np.full(((n + 63) // 64, 8), SENT, np.float32)
    flagged = (flags & F_DEMO) != 0
    grp = D.group_of(np.arange(n), epg)
    for g in np.unique(grp):
        sel = np.nonzero(flagged & (grp == g))[0]
        if len(sel):
            r_out[sel] = D.reward(gt[sel], D.min2(sets[g], ns[sel]), (flags[sel] & F_STUCK) != 0)
    slot = (base + np.arange(n)) % cap
    rows[slot[flagged], 4] = r_out[flagged].astype(np.float32)
    for k in range(len(stats)):
        e = np.arange(64 * k, 64 * k + 64)
        live = e < n
        if flagged[e[live]].any():
            lanes = np.zeros(64, np.float32)
            lanes[live] = rows[slot[e[live]], 4]
            stats[k, 0] = D.wave_sum32(lanes)
    return rows, r_out, stats


def check_reward_pass(form, lay, ns, gt, flags, epg):
    got = reward_pass(form, lay, ns, gt, flags, epg)
    want = reward_expected(lay, ns, gt, flags, epg)
    for name, a, b in zip(("rows", "reward_out", "block_stats"), got, want):
        assert np.array_equal(a, b), (form, name, np.nonzero(a != b)[0][:8])
    return got


@pytest.mark.parametrize("form", ["brute", "indexed"])
def test_reward_passes_on_ragged_groups(lay, form):
    """nav_demo_reward (k_demo_reward: one-group waves split 8 ways over 1, 3, 70, 11 355 and 17
    points, and mixed-group waves) and nav_demo_reward_indexed (lists of 1 .. 28 and 17 entries)
    with flags the test writes: every flagged env's reward, no exclusions."""
    rng = np.random.default_rng(5)
    flags = written_flags(N, rng)
    gt = -rng.uniform(0, 120, N)
    _, r, _ = check_reward_pass(form, lay, lay["s"], gt, flags, EPG)
    assert np.isfinite(r).all() and ((flags & F_DEMO) != 0).sum() > N // 2


@pytest.mark.parametrize("form", ["brute", "indexed"])
@pytest.mark.parametrize("n", [5, 8, 9])
def test_reward_passes_few_envs(lay, form, n):
    """n <= 8: k_demo_reward_few (a lane per point) with per-group offsets, 2 envs per group;
    n = 9: the other side of the switch, a wave kernel launch of one mixed-group wave."""
    rng = np.random.default_rng(50 + n)
    e = np.arange(n)
    ns = lay["s"][(e // 2) * EPG + 3 * (e % 2) + 3 + n]  # states of the env's own group
    flags = written_flags(n, rng)
    check_reward_pass(form, lay, ns, -rng.uniform(0, 120, n), flags, 2)


@pytest.mark.parametrize("form", ["brute", "indexed"])
def test_reward_passes_outside_the_index(lay, form):
    """Caller-supplied next states outside [0,100)^2 (x or y = -0.5, exactly 100.0, 250.0) among
    states inside it, grouped form: the indexed pass leaves its lists for the brute force over
    the env's group, the brute pass never had an index."""
    rng = np.random.default_rng(6)
    ns = lay["s"].copy()
    out = np.array([-0.5, 100.0, 250.0])
    k = 0
    for e in range(N):
        if e % 3 == 1:
            continue
        which = k % 3  # x, y, both
        if which != 1:
            ns[e, 0] = out[(k // 3) % 3]
        if which != 0:
            ns[e, 1] = out[(k // 9) % 3]
        k += 1
    assert (~D.in_index(ns)).sum() > N // 2 and D.in_index(ns).sum() > N // 4
    flags = written_flags(N, rng)
    _, r, _ = check_reward_pass(form, lay, ns, -rng.uniform(0, 120, N), flags, EPG)
    assert np.isfinite(r).all()


def test_shared_set_outside_the_index_through_vecenv(lay):
    """A shared demo set (no offsets) through VecEnv's two-launch indexed path with next_state
    overwritten by out-of-world values: VecEnv hands the indexed entry points the set as one
    group {0, m}, so the fallback has the set's m points, and the reward equals demo_ref's
    (with demo_off == NULL the entry point has no m: -inf)."""
    from nav.vec_env import ReplayRing, VecEnv
    P = sets_of(lay)[3]
    n = 300
    env = VecEnv(n, lay["field"], seed=3, envs_per_group=64)
    env.set_demo(P)
    env.fuse_demo = False
    assert env.demo_off is None
    rep = ReplayRing(n + 3, DEV)
    rep.position = 7
    r_out = torch.full((n,), SENT, dtype=torch.float64, device=DEV)
    base = env.agent_step(torch.zeros(n, 2, dtype=torch.float64, device=DEV), rep, reward_out=r_out)
    ns = env.next_state.cpu().numpy()
    out = np.array([-0.5, 100.0, 250.0])
    for e in range(0, n, 2):
        k = e // 2
        if k % 3 != 1:
            ns[e, 0] = out[(k // 3) % 3]
        if k % 3 != 0:
            ns[e, 1] = out[(k // 9) % 3]
    assert (~D.in_index(ns)).sum() == n // 2
    env.next_state.copy_(dev(ns))
    r_out.fill_(SENT)
    env.demo_reward(rep, base, reward_out=r_out)
    torch.cuda.synchronize()
    flags = env.flags.cpu().numpy()
    flagged = (flags & F_DEMO) != 0
    assert flagged.sum() > n // 2
    want = np.full(n, SENT)
    want[flagged] = D.reward(env.goal_term.cpu().numpy()[flagged], D.min2(P, ns[flagged]),
                             (flags[flagged] & F_STUCK) != 0)
    assert np.isfinite(want).all()
    assert np.array_equal(r_out.cpu().numpy(), want)
    slot = (base + np.arange(n)) % rep.capacity
    assert np.array_equal(rep.rows.cpu().numpy()[slot[flagged], 4], want[flagged].astype(np.float32))


# ---------------------------------------------------------------- the ticks
SEED = 21


def tick_inputs(lay, demo_only=None):
    """goal, meta and the stuck ring for the query states: every 11th env within reach of its
    goal (no demo term), every 7th without the demo flag (demo_only = (k, r): the demo flag on
    the envs e % k == r alone), every 5th with a full ring of its own state (stuck on this
    tick); every other goal 30 away"""
    s = lay["s"]
    n = lay["n"]
    e = np.arange(n)
    goal = s + np.stack([np.where(s[:, 0] < 50.0, 30.0, -30.0), np.zeros(n)], 1)
    near = e % 11 == 0
    goal[near] = s[near] + np.array([1.0, -1.0])
    demo = e % 7 != 0 if demo_only is None else e % demo_only[0] == demo_only[1]
    meta = np.where(demo, 4, 0) | np.where(e % 5 == 0, 5 << 8, 0)
    hist = np.tile(s[None], (5, 1, 1))
    return goal, meta.astype(np.int32), hist


def run_tick(lay, form, action=None, actor=None, demo_only=None):
    """One tick of a layout from its query states in one launch form: "fused"
    (nav_agent_step_indexed), "per_env" (nav_agent_step + nav_demo_reward_indexed), "brute"
    (nav_agent_step + nav_demo_reward) or, with an actor, nav_act_tick. Returns every output."""
    from nav.vec_env import ReplayRing, VecEnv
    N = lay["n"]
    env = VecEnv(N, lay["field"], seed=SEED, envs_per_group=EPG)
    env.set_demo(lay["pts"], lay["off"], index=form != "brute")
    env.fuse_demo = form == "fused"
    goal, meta, hist = tick_inputs(lay, demo_only)
    env.state.copy_(dev(lay["s"]))
    env.goal.copy_(dev(goal))
    env.meta.copy_(dev(meta))
    env.hist.copy_(dev(hist))
    env.block_stats.fill_(SENT)
    rep = ReplayRing(N + 3, DEV)
    rep.position = 7
    rep.rows.fill_(SENT)
    r_out = torch.full((N,), SENT, dtype=torch.float64, device=DEV)
    a_out = None
    if actor is not None:
        a_out = torch.zeros(N, 2, dtype=torch.float64, device=DEV)
        base = env.act_tick(actor, 3, rep, action_out=a_out, reward_out=r_out)
    else:
        if action is None:
            action = torch.zeros(N, 2, dtype=torch.float64, device=DEV)
        base = env.agent_step(action, rep, reward_out=r_out)
    torch.cuda.synchronize()
    assert base == 7
    out = {k: getattr(env, k).cpu().numpy() for k in (
        "next_state", "goal_term", "flags", "block_stats", "state", "meta", "plan_index",
        "path_length", "episodes", "noise_scale", "hist")}
    out.update(rows=rep.rows.cpu().numpy(), reward_out=r_out.cpu().numpy())
    if a_out is not None:
        out["action"] = a_out
    return out


def same_bits(a, b, what):
    for k in a:
        if k != "action":
            assert np.array_equal(a[k], b[k]), (what, k)


def check_tick_against_reference(lay, o):
    """every env carrying F_DEMO against demo_ref on the next_state the tick published; the
    other envs' pushed reward from their own flags. Returns the flagged share per group."""
    sets = sets_of(lay)
    fl, ns, gt = o["flags"], o["next_state"], o["goal_term"]
    flagged = (fl & F_DEMO) != 0
    stuck = (fl & F_STUCK) != 0
    N = lay["n"]
    grp = D.group_of(np.arange(N))
    want = np.where((fl & 2) != 0, 50.0, gt) - np.where(stuck, 50.0, 0.0)
    for g in range(lay["G"]):
        sel = np.nonzero(flagged & (grp == g))[0]
        want[sel] = D.reward(gt[sel], D.min2(sets[g], ns[sel]), stuck[sel])
    assert np.array_equal(o["reward_out"][flagged], want[flagged])
    assert (o["reward_out"][~flagged] == SENT).all()
    slot = (7 + np.arange(N)) % (N + 3)
    assert np.array_equal(o["rows"][slot, 4], want.astype(np.float32))
    assert D.in_index(ns).all()
    return [flagged[grp == g].mean() for g in range(lay["G"])]


def test_tick_launch_forms_on_ragged_groups(lay):
    """nav_agent_step_indexed (the block's demo pass over per-slot group offsets, slots past n,
    lists of 1 and of 17) and nav_agent_step + either reward pass, zero actions: rows, flags,
    rewards, block_stats and the env state bit for bit among the forms, flagged envs against
    demo_ref. Flagged share per group (seed 21, observed): A 0.781, B 0.771, C 0.771, D 0.792,
    E 0.779 (every 7th env has no demo flag, every 11th reaches its goal)."""
    fused, per_env, brute = (run_tick(lay, f) for f in ("fused", "per_env", "brute"))
    same_bits(fused, brute, "fused")
    same_bits(per_env, brute, "per_env")
    share = check_tick_against_reference(lay, fused)
    print("flagged share per group:", ["%.3f" % x for x in share])
    assert min(share) >= 0.25
    fl = fused["flags"]
    assert ((fl & F_DEMO) != 0)[(fl & F_STUCK) != 0].any()  # stuck and flagged on one tick
    assert (fl & 2).any() and (fl & 8).any()                # goal hits, ended episodes
    assert (fused["block_stats"][:, 0] != SENT).all() and (fused["block_stats"][:, 5:] == 0).all()


def test_act_tick_on_ragged_groups(lay):
    """nav_act_tick (the demo pass behind the actor GEMM; hidden 64 x 1 layer) with action_out,
    then those actions through nav_agent_step + nav_demo_reward (brute) on an identical env:
    bit for bit, and the flagged envs against demo_ref. Flagged share per group (observed):
    A 0.802, B 0.771, C 0.781, D 0.792, E 0.779."""
    from nav.mlp import DeviceMLP
    from oracle.td3_oracle import make_mlp_params
    actor = DeviceMLP(2, 2, 64, 1, DEV).load(make_mlp_params(8, [2, 64, 2]))
    fused = run_tick(lay, "fused", actor=actor)
    a = fused["action"]
    assert torch.isfinite(a).all() and (a != 0).any()
    brute = run_tick(lay, "brute", action=a)
    same_bits(fused, brute, "act_tick")
    share = check_tick_against_reference(lay, fused)
    print("flagged share per group:", ["%.3f" % x for x in share])
    assert min(share) >= 0.25


def test_tick_demo_pass_with_few_flagged_envs(lay):
    """The block's demo pass with most slots of length 0: the demo flag on every 13th env alone
    (an extra case; the share bound above is for the issue's flagging)."""
    fused, brute = (run_tick(lay, f, demo_only=(13, 5)) for f in ("fused", "brute"))
    same_bits(fused, brute, "fused")
    check_tick_against_reference(lay, fused)
    flagged = (fused["flags"] & F_DEMO) != 0
    assert 20 <= flagged.sum() <= N // 13 + 1


# ---------------------------------------------------------------- long lists
def test_ring_index_build_equals_reference(ring):
    """Every cell of both groups of the ring layout, and that its lists are long: up to all 300
    points of the circle, and the first workgroup's lists together several trips of the demo
    pass (256 threads x 8 entries per trip)."""
    ix = {k: v.cpu().numpy() for k, v in ring["ix"].items()}
    check_scans(ring, ix)
    l2 = check_index_group(ring, ix, 0, None)
    check_index_group(ring, ix, 1, None)
    lens = l2.count[D.index_cell(ring["s"][:EPG], ring["res"])]
    assert lens.max() == 300 and lens.sum() > 4 * 256 * 8


@pytest.mark.parametrize("form", ["brute", "indexed"])
def test_ring_reward_passes(ring, form):
    rng = np.random.default_rng(15)
    n = ring["n"]
    flags = written_flags(n, rng)
    check_reward_pass(form, ring, ring["s"], -rng.uniform(0, 120, n), flags, EPG)


def test_ring_tick_launch_forms(ring):
    """The tick's launch forms on lists of about 300 entries per flagged env: the block's demo
    pass takes several trips, a thread's 8 entries span list ends, and per-env minima meet in
    the LDS atomic min from many threads."""
    from nav.mlp import DeviceMLP
    from oracle.td3_oracle import make_mlp_params
    fused, per_env, brute = (run_tick(ring, f) for f in ("fused", "per_env", "brute"))
    same_bits(fused, brute, "fused")
    same_bits(per_env, brute, "per_env")
    share = check_tick_against_reference(ring, fused)
    assert min(share) >= 0.25
    actor = DeviceMLP(2, 2, 64, 1, DEV).load(make_mlp_params(8, [2, 64, 2]))
    acted = run_tick(ring, "fused", actor=actor)
    same_bits(acted, run_tick(ring, "brute", action=acted["action"]), "act_tick")
    check_tick_against_reference(ring, acted)
