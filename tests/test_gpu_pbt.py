"""Population-based training on the GPU: the members' scores in one launch
(nav_pop_test_summary) against torch and numpy, the cloning of learners in one launch
(nav_td3_pop_exploit) as a byte copy that touches nothing else, and the trainer's exploit /
explore / pbt_step on top of them. Copies are compared bitwise (torch.equal)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gpu_support import nav  # noqa: F401
from pop_support import (CAP, DEV, FILL, copied_state, differences, equal_tree, learner_state,
                         leaves, make_ring, make_td3, member_state, state_member, workspace)

pytestmark = pytest.mark.gpu


# ---- 1. the summary
def summarise(reached, steps, best, P, epm):
    """nav_pop_test_summary's [P] structs as raw bytes per member."""
    from nav._lib import NavPopScore, NavTestOut, lib, ptr, stream_handle
    size = C.sizeof(NavPopScore)
    buf = torch.zeros(P * size, dtype=torch.uint8, device=DEV)
    o = NavTestOut(ptr(reached), ptr(steps), ptr(best), None, None)
    lib().nav_pop_test_summary(C.byref(o), P, epm, ptr(buf), stream_handle())
    raw = buf.cpu().numpy().tobytes()
    return [raw[m * size:(m + 1) * size] for m in range(P)]


@pytest.mark.parametrize("epm", [192, 64])
def test_summary_against_torch(nav, epm):
    """P = 3: member 0 has none reached, member 1 all, member 2 some. The integer fields and the
    maximum are exact; the sum is within what two summation orders of n non-negative doubles can
    differ by, (n - 1) 2^-52 sum; a second call and the same slice as a population of one give
    the same bits."""
    from nav._lib import NavPopScore
    P = 3
    g = torch.Generator().manual_seed(40 + epm)
    reached = torch.zeros(P, epm, dtype=torch.uint8)
    reached[1] = 1
    reached[2] = (torch.rand(epm, generator=g) < 0.4).to(torch.uint8)
    assert 0 < int(reached[2].sum()) < epm
    steps = torch.randint(1, 1001, (P, epm), generator=g, dtype=torch.int32)
    best = torch.rand(P, epm, generator=g, dtype=torch.float64) * 140.0
    d = [t.reshape(-1).contiguous().to(DEV) for t in (reached, steps, best)]
    raw = summarise(*d, P, epm)
    for m in range(P):
        s = NavPopScore.from_buffer_copy(raw[m])
        hit = reached[m].bool()
        assert s.reached == int(hit.sum())
        assert s.steps_reached == int(steps[m][hit].long().sum())
        assert s.max_best == best[m].max().item()
        # and torch's own reductions on the device, as evaluate() takes them
        assert s.max_best == d[2][m * epm:(m + 1) * epm].max().item()
        want = float(np.sum(best[m].numpy()))
        print(f"epm {epm} member {m}: sum_best {s.sum_best!r} numpy {want!r} "
              f"diff {abs(s.sum_best - want):.3e} bound {(epm - 1) * 2.0 ** -52 * want:.3e}")
        assert abs(s.sum_best - want) <= (epm - 1) * 2.0 ** -52 * want
    assert summarise(*d, P, epm) == raw
    sl = slice(epm, 2 * epm)
    one = summarise(d[0][sl], d[1][sl], d[2][sl], 1, epm)
    assert one[0] == raw[1]
    two = summarise(d[0][epm:], d[1][epm:], d[2][epm:], 2, epm)
    assert two == raw[1:]


# ---- 2. the exploit launch
SHAPES = [(64, 2), (200, 3), (32, 1), (256, 2)]


@pytest.mark.parametrize("hidden,nh", SHAPES, ids=[f"h{h}x{n}" for h, n in SHAPES])
def test_exploit_is_a_byte_copy_and_touches_nothing_else(nav, hidden, nh):
    """Four distinct learners after three epochs; src = [0, 0], dst = [2, 3], 3 000 of 4 096 ring
    rows: members 2 and 3 hold member 0's parameters, images, moments and first 3 000 rows, their
    later rows and workspaces are as before, members 0 and 1 are untouched. Then one pair with
    replay_rows = 0: the ring stays."""
    from nav._lib import NavTd3Member, lib, ptr, stream_handle
    P, B = 4, 100
    rings = [make_ring(m) for m in range(P)]
    for m, r in enumerate(rings):  # rows no learner reads, distinct per member
        r.rows[FILL:] = float(m + 1)
    td3 = [make_td3(m, hidden, nh, B, 3) for m in range(P)]
    for t, r in zip(td3, rings):
        t.td3_update(r, 3)
    torch.cuda.synchronize()
    before = [copied_state(t) for t in td3]
    rows0 = [r.rows.clone() for r in rings]
    work0 = [workspace(t) for t in td3]
    # a condition of the test: every copied buffer differs between any two members (one hidden
    # layer has no image: its `packed` is a placeholder the library does not look at)
    for a in range(P):
        for b in range(a + 1, P):
            same = [p for (p, x), (_, y) in zip(leaves(before[a]), leaves(before[b]))
                    if torch.equal(x, y) and not (nh == 1 and p.startswith("/packed"))]
            assert not same, (a, b, same)
            assert not torch.equal(rows0[a][:FILL], rows0[b][:FILL])
            assert not torch.equal(rows0[a][FILL:], rows0[b][FILL:])
            assert not torch.equal(work0[a]["batch"], work0[b]["batch"])

    L, s = lib(), stream_handle()
    arr = (NavTd3Member * P)(*[state_member(t, r) for t, r in zip(td3, rings)])
    tab = torch.zeros(L.nav_td3_pop_state_bytes(P), dtype=torch.uint8, device=DEV)
    L.nav_td3_pop_state_build(arr, P, ptr(tab), s)
    i32 = lambda v: (C.c_int32 * len(v))(*v)  # noqa: E731
    L.nav_td3_pop_exploit(arr, P, ptr(tab), i32([0, 0]), i32([2, 3]), 2, FILL, s)
    torch.cuda.synchronize()
    for m in (2, 3):
        equal_tree(copied_state(td3[m]), before[0], f"member {m} is member 0")
        assert torch.equal(rings[m].rows[:FILL], rows0[0][:FILL])
        assert torch.equal(rings[m].rows[FILL:], rows0[m][FILL:])
        equal_tree(workspace(td3[m]), work0[m], f"member {m}'s workspace")
    for m in (0, 1):
        equal_tree(copied_state(td3[m]), before[m], f"member {m} untouched")
        assert torch.equal(rings[m].rows, rows0[m])
        equal_tree(workspace(td3[m]), work0[m], f"member {m}'s workspace")

    # replay_rows = 0: member 2 becomes member 1, every ring stays
    rows1 = [r.rows.clone() for r in rings]
    L.nav_td3_pop_exploit(arr, P, ptr(tab), i32([1]), i32([2]), 1, 0, s)
    torch.cuda.synchronize()
    equal_tree(copied_state(td3[2]), before[1], "member 2 is member 1")
    equal_tree(copied_state(td3[3]), before[0], "member 3 stays member 0")
    for m in range(P):
        assert torch.equal(rings[m].rows, rows1[m])
    # the whole ring
    L.nav_td3_pop_exploit(arr, P, ptr(tab), i32([1]), i32([0]), 1, CAP, s)
    torch.cuda.synchronize()
    assert torch.equal(rings[0].rows, rows1[1])
    equal_tree(copied_state(td3[0]), before[1], "member 0 is member 1")


def test_state_table_past_one_chunk(nav):
    """Seven distinct learners at hidden 32 x 1, batch 64, after one epoch: the smallest
    population whose state table (7 entries of 304 B) spans two of the table writer's 2 KB chunks,
    the second one partial and member 6's entry across the boundary. src = [0, 1], dst = [6, 5],
    3 000 ring rows: members 6 and 5 are byte copies of members 0 and 1, the others are
    untouched."""
    from nav._lib import NavTd3Member, lib, ptr, stream_handle
    P, B = 7, 64
    rings = [make_ring(m) for m in range(P)]
    td3 = [make_td3(m, 32, 1, B, 1) for m in range(P)]
    for t, r in zip(td3, rings):
        t.td3_update(r, 1)
    torch.cuda.synchronize()
    before = [copied_state(t) for t in td3]
    rows0 = [r.rows.clone() for r in rings]
    for a in range(P):  # a condition of the test: every copied buffer differs between members
        for b in range(a + 1, P):
            same = [p for (p, x), (_, y) in zip(leaves(before[a]), leaves(before[b]))
                    if torch.equal(x, y) and not p.startswith("/packed")]
            assert not same, (a, b, same)
            assert not torch.equal(rows0[a][:FILL], rows0[b][:FILL])
    L, s = lib(), stream_handle()
    arr = (NavTd3Member * P)(*[state_member(t, r) for t, r in zip(td3, rings)])
    nbytes = L.nav_td3_pop_state_bytes(P)
    assert nbytes > 2048 and nbytes % 2048 != 0
    tab = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    L.nav_td3_pop_state_build(arr, P, ptr(tab), s)
    i32 = lambda v: (C.c_int32 * len(v))(*v)  # noqa: E731
    L.nav_td3_pop_exploit(arr, P, ptr(tab), i32([0, 1]), i32([6, 5]), 2, FILL, s)
    torch.cuda.synchronize()
    for d, src in ((6, 0), (5, 1)):
        equal_tree(copied_state(td3[d]), before[src], f"member {d} is member {src}")
        assert torch.equal(rings[d].rows[:FILL], rows0[src][:FILL])
        assert torch.equal(rings[d].rows[FILL:], rows0[d][FILL:])
    for m in range(5):
        equal_tree(copied_state(td3[m]), before[m], f"member {m} untouched")
        assert torch.equal(rings[m].rows, rows0[m])


# ---- 3 .. 6. the trainer
TRAINER = dict(envs_per_member=128, hidden=64, n_hidden=2, batch=128, updates_per_step=2,
               seed=1234, envs_per_group=128, replay_capacity=1024, demos=False)


def trainer(members, **kw):
    from nav.population import PopulationTrainer
    return PopulationTrainer(members, device=DEV, **{**TRAINER, **kw})


@pytest.mark.parametrize("learner", ["members", "batched"])
def test_a_clone_continues_as_its_source(nav, learner):
    """Two members with the same learner seed on their own envs: after 4 steps they differ; after
    exploit([0], [1]) one learn() alone (no tick) leaves member 1's networks, images, moments,
    sampled batches and every workspace buffer bit-equal to member 0's: a buffer the copy missed
    would show."""
    tr = trainer([{"seed": 7}, {"seed": 7}], learner=learner)
    for _ in range(4):
        tr.step()
    torch.cuda.synchronize()
    a, b = learner_state(tr.td3[0], work=True), learner_state(tr.td3[1], work=True)
    differ = differences(a, b)
    for kind in ("params", "packed"):
        for k in a[kind]:
            assert f"/{kind}/{k}" in differ, (kind, k)
    for k in a["adam"]:
        assert f"/adam/{k}/m" in differ and f"/adam/{k}/v" in differ, k
    assert "/work/batch" in differ and not torch.equal(tr.rings[0].rows, tr.rings[1].rows)
    assert tr.td3[0].update_counter == 8
    tr.exploit([0], [1], copy_replay=True)
    tr.learn()
    torch.cuda.synchronize()
    assert tr.td3[0].update_counter == 10
    equal_tree(learner_state(tr.td3[1], work=True), learner_state(tr.td3[0], work=True))
    assert torch.equal(tr.rings[0].rows, tr.rings[1].rows)
    assert differences(learner_state(tr.td3[0], work=True), a)  # and the learners moved


def test_the_others_are_untouched(nav):
    """Three members, 4 steps, exploit([0], [2]) with an explore on critic_lr, 4 more steps,
    against the same run without the exploit: members 0 and 1 end bit-equal (env slice, ring,
    learner), member 2 differs."""
    members = [{"critic_lr": 1e-3}, {"critic_lr": 5e-4}, {"seed": 11}]

    def run(exploit):
        tr = trainer(members)
        for _ in range(4):
            tr.step()
        if exploit:
            tr.exploit([0], [2], explore={"critic_lr": (1e-5, 1e-2)},
                       rng=np.random.default_rng(5))
        for _ in range(4):
            tr.step()
        torch.cuda.synchronize()
        return tr, [member_state(tr, m) for m in range(3)]

    ta, a = run(True)
    _, b = run(False)
    equal_tree(a[0], b[0], "member 0")
    equal_tree(a[1], b[1], "member 1")
    assert not torch.equal(a[2]["td3"]["critic1"]["params"], b[2]["td3"]["critic1"]["params"])
    assert not torch.equal(a[2]["td3"]["actor"]["params"], b[2]["td3"]["actor"]["params"])
    # the clone's envs went on from their own state with the new policy; its seed is its own
    assert ta.td3[2].seed == 11 and ta.members[2]["seed"] == 11
    assert ta.members[2]["critic_lr"] in (1e-3 * 0.8, 1e-3 * 1.25)


def test_explore_reaches_host_and_device(nav):
    tr = trainer([{}, {}])
    lr0 = tr.td3[0].cfg.critic_lr
    tr.exploit([0], [1], explore={"max_action": (1.0, 1.0), "critic_lr": (1e-5, 1e-2)})
    new_lr = tr.members[1]["critic_lr"]
    assert new_lr in (lr0 * 0.8, lr0 * 1.25)
    assert tr.members[1]["max_action"] == 1.0
    assert tr.params[1].max_action == 1.0 and tr.pop.params[1].max_action == 1.0
    assert tr.td3[1].cfg.max_action == 1.0 and tr.td3[1].cfg.critic_lr == new_lr
    assert tr.td3[1].critic_optimizer_1.lr == new_lr == tr.td3[1].critic_optimizer_2.lr
    assert tr.td3[0].cfg.critic_lr == lr0 and tr.td3[0].critic_optimizer_1.lr == lr0
    assert tr.params[0].max_action == 5.0 and tr.members[0] == {}
    ev = tr.pbt_history[-1]
    assert len(tr.pbt_history) == 1 and (ev["step"], ev["src"], ev["dst"]) == (0, 0, 1)
    assert ev["before"] == {"max_action": 5.0, "critic_lr": lr0}
    assert ev["after"] == {"max_action": 1.0, "critic_lr": new_lr}
    with pytest.raises(KeyError, match="cannot be explored"):
        tr.exploit([0], [1], explore={"policy_update_delay": (1, 4)})
    assert len(tr.pbt_history) == 1
    tr.collect()
    torch.cuda.synchronize()
    a0 = tr.action[tr.member_slice(0)].abs().max().item()
    a1 = tr.action[tr.member_slice(1)].abs().max().item()
    # the condition: the world is 100 wide, so the baseline action saturates at member 0's 5
    assert a0 > 1.0
    assert a1 <= 1.0


SCORE_KEYS = {"n", "reached", "success_rate", "mean_steps_reached", "mean_best_distance",
              "max_best_distance", "max_steps", "episode"}


def test_scores_agree_with_evaluate(nav):
    """P = 2, 64-step episodes, 128 envs per member (a power of two: the division of either sum
    by n is exact, so the means differ by the sums' bound over n)."""
    from nav import pbt_select
    tr = trainer([{"demo_factor": 10.0}, {"demo_factor": 30.0, "seed": 3}])
    for _ in range(2):
        tr.step()
    n = tr.epm
    ev = tr.evaluate(max_steps=64)
    sc = tr.scores(max_steps=64)
    assert len(sc) == len(ev) == 2
    for m, (s, e) in enumerate(zip(sc, ev)):
        assert set(s) == SCORE_KEYS | set(tr.members[m])
        assert s["success_rate"] * n == e["success_rate"] * n == s["reached"]
        assert s["max_best_distance"] == e["max_best_distance"]
        bound = (n - 1) * 2.0 ** -52 * e["mean_best_distance"]
        print(f"member {m}: mean_best_distance scores {s['mean_best_distance']!r} evaluate "
              f"{e['mean_best_distance']!r} bound {bound:.3e}")
        assert abs(s["mean_best_distance"] - e["mean_best_distance"]) <= bound
        if s["reached"]:
            assert math.isclose(s["mean_steps_reached"], e["mean_steps_reached"], rel_tol=1e-15)
        else:
            assert math.isnan(s["mean_steps_reached"]) and math.isnan(e["mean_steps_reached"])
        assert (s["n"], s["max_steps"], s["episode"]) == (n, 64, 0)
        assert s["demo_factor"] == tr.members[m]["demo_factor"]
    got, (src, dst) = tr.pbt_step(max_steps=64)
    assert (src, dst) == pbt_select(got, frac=0.25)
    assert len(dst) == 1 and len(tr.pbt_history) == 1
    assert [{k: v for k, v in g.items() if k != "mean_steps_reached"} for g in got] == \
        [{k: v for k, v in s.items() if k != "mean_steps_reached"} for s in sc]
    # the clone reports its source's demo_factor from now on, and keeps its seed
    assert tr.members[dst[0]]["demo_factor"] == tr.members[src[0]]["demo_factor"]
    assert tr.members[1].get("seed") == 3 and "seed" not in tr.members[0]
