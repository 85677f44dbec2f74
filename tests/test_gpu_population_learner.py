"""The population learner on the GPU: every member's TD3 epochs in one launch per kernel
(nav.population.PopulationLearner over nav_td3_critic_rows_pop, nav_mlp_wgrad_pop,
nav_grad_reduce_adam_pop, nav_td3_actor_rows_pop) against the single-member path, which the rest
of the suite pins to the oracle and the reference's gradients. Every comparison is bitwise
(torch.equal): a member of the batched form runs the same device code on the same data as a lone
TD3 with the same weight-gradient split counts."""
import pytest
import torch

from gpu_support import nav  # noqa: F401
from pop_support import (DEV, equal_tree, injection, learner_state, make_ring, make_td3,
                         member_state)

pytestmark = pytest.mark.gpu


def run_case(P, hidden, nh, B, epochs, inject=False):
    """(batched states, lone states, the learner): P distinct members through `epochs` epochs of
    the batched form, and P lone TD3 objects with the batched run's split counts from the same
    initial state (same seeds) on the same rings."""
    from nav.population import PopulationLearner
    rings = [make_ring(m) for m in range(P)]
    td3 = [make_td3(m, hidden, nh, B, epochs) for m in range(P)]
    learner = PopulationLearner(td3, rings)
    inj = [injection(m, B) for m in range(P)] if inject else None
    if inject:
        learner.inject(idx_critic=[i[0] for i in inj], idx_actor=[i[1] for i in inj],
                       eps=[i[2] for i in inj])
    learner.update(epochs)
    torch.cuda.synchronize()
    got = [learner_state(t) for t in td3]
    want = []
    for m in range(P):
        t = make_td3(m, hidden, nh, B, epochs, splits=learner.wgrad_splits)
        if inject:
            ic, ia, eps = inj[m]
            # td3_update draws idx_fn for the critic batch, then (policy epochs: 0, 2, ...) for
            # the actor batch
            seq = iter([x for e in range(epochs) for x in ([ic, ia] if e % 2 == 0 else [ic])])
            t.td3_update(rings[m], epochs, idx_fn=lambda: next(seq), eps_fn=lambda: eps)
        else:
            t.td3_update(rings[m], epochs)
        torch.cuda.synchronize()
        assert (t.splits_c, t.splits_a) == learner.wgrad_splits
        want.append(learner_state(t))
    return got, want, learner


def check_case(got, want):
    for m, (g, w) in enumerate(zip(got, want)):
        equal_tree(g, w, f"member {m}")
    # a condition of the test: the members differ, so another member's table entry cannot pass
    for m in range(1, len(got)):
        for k in ("actor", "critic1", "critic2", "target_actor", "target_critic1"):
            assert not torch.equal(got[0]["params"][k], got[m]["params"][k]), (m, k)
        assert not torch.equal(got[0]["batch"], got[m]["batch"])
        assert not torch.equal(got[0]["da"], got[m]["da"])
    # and the learner ran: parameters moved and every counter advanced
    assert all(g["update_counter"] == want[0]["update_counter"] > 0 for g in got)


CASES = [(64, 2, 100),     # partial last row block, the reference's batch, split twins
         (256, 2, 2112),   # unsplit twins, the 256 x 32 factored weight-gradient tiles
         (200, 3, 100),    # hp 224, saved middle layers, k_wgrad_gen
         (32, 1, 100),     # no hidden x hidden weights, no pack
         # the mlp_lpop objects of NT = hidden_pad / 32 = 3 .. 6
         (90, 2, 100), (128, 2, 100), (150, 3, 100), (192, 2, 100)]


@pytest.mark.parametrize("hidden,nh,B", CASES, ids=[f"h{h}x{n}_b{b}" for h, n, b in CASES])
def test_epochs_distinct_members(nav, hidden, nh, B):
    """P = 3, three epochs (0 and 2 policy epochs, 1 critic only): per member the parameters,
    packed images and Adam moments of the three online nets, the three targets, both sampled
    batches, dq, loss_part, q, da and the counters equal the lone TD3's."""
    got, want, learner = run_case(3, hidden, nh, B, 3)
    check_case(got, want)
    assert got[0]["update_counter"] == 3
    assert got[0]["adam"]["critic1"]["t"] == 3 and got[0]["adam"]["actor"]["t"] == 2


def test_epochs_injected_samples(nav):
    """The same with each member's own injected sample indices and smoothing noise: the table's
    nullable idx / eps pointers."""
    got, want, _ = run_case(3, 64, 2, 100, 3, inject=True)
    check_case(got, want)
    ic, _, _ = injection(1, 100)
    # a condition: the injected indices were used (member 1's batch is its ring's rows at them)
    ring = make_ring(1)
    assert torch.equal(got[1]["batch"], ring.rows[ic])


def test_coresident_grid(nav):
    """P = 8 at hidden 256 x 2, batch 2112, one policy epoch and one critic-only epoch: more row
    workgroups than CUs in one launch, members' workgroups co-resident on a CU."""
    got, want, _ = run_case(8, 256, 2, 2112, 2)
    check_case(got, want)


# ---- the trainer
TRAINER = dict(hidden=64, n_hidden=2, batch=128, updates_per_step=2, seed=1234,
               envs_per_group=128)


equal_any = equal_tree


def run_trainer(members, **kw):
    from nav.population import PopulationTrainer
    tr = PopulationTrainer(members, envs_per_member=256, device=DEV, **TRAINER, **kw)
    for _ in range(6):
        tr.step()
    torch.cuda.synchronize()
    return tr, [member_state(tr, m) for m in range(len(members))]


def test_trainer_one_member_is_vectrainer(nav):
    """learner="batched" with one member after 6 steps equals VecTrainer with the same arguments:
    env, ring, every parameter and moment."""
    from nav.trainer import VecTrainer
    pt, st = run_trainer([{}], learner="batched")
    vt = VecTrainer(n_envs=256, device=DEV, **TRAINER)
    for _ in range(6):
        vt.step()
    torch.cuda.synchronize()
    sd = vt.state_dict()
    want = {"env": sd["env"], "replay": sd["replay"], "td3": sd["td3"],
            "steps": sd["meta"]["steps"]}
    equal_any(st[0], want)
    assert pt.td3[0].update_counter == 12


def test_trainer_batched_is_members_and_isolates(nav):
    """P = 2: the batched learner equals learner="members" with the batched run's split counts for
    both members; changing only member 1's critic_lr leaves member 0 bit-identical and changes
    member 1."""
    bt, b = run_trainer([{}, {}], learner="batched")
    _, a = run_trainer([{}, {}], learner="members", wgrad_splits=bt.learner.wgrad_splits)
    equal_any(b, a)
    ct, c = run_trainer([{}, {"critic_lr": 1e-4}], learner="batched")
    equal_any(c[0], b[0])
    assert not torch.equal(c[1]["td3"]["critic1"]["params"], b[1]["td3"]["critic1"]["params"])
    assert all(t.update_counter == 12 for t in bt.td3 + ct.td3)
