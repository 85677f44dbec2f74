"""Population training: P members, each with its own actor, twin critics and learner, its own
replay ring and its own `nav_params`, on ONE env set, acting and ticking in ONE launch and running
their test episodes in ONE launch (nav_act_tick_pop / nav_test_rollout_pop).

The reference's only published result is a hyper-parameter study (the score over
DEMO_PROXIMITY_FACTOR in {10, 30, 50, 70}; simulator.py:169-200 attempts the same over
INITIAL_NOISE x NOISE_DECAY). Envs are independent of each other (environment.py:98-137), so a
sweep is a population: member m owns the consecutive envs [m * envs_per_member, (m + 1) *
envs_per_member) and ends exactly as it would alone on the whole env set, bit for bit.

The learner has two forms. learner="members" (the default): each member's td3_update runs the
single-member kernels at its batch size, optionally round-robin over a few streams.
learner="batched" (PopulationLearner): every member's TD3 epoch in one launch per kernel
(nav_td3_critic_rows_pop, nav_mlp_wgrad_pop, nav_grad_reduce_adam_pop, nav_td3_actor_rows_pop):
the same kernels with a member dimension on the grid, member m's arguments read from a device
table built once, the replay fill, the Philox counter and Adam's bias corrections by value. Member
m ends bit for bit as its own td3_update with the same weight-gradient split counts; those are
chosen to fill the chip with all members' tiles, so for P > 1 they differ from a lone learner's
(wgrad_splits= sets up a "members" run to match).

Population-based training turns the grid into a search: scores() reduces every member's test
episodes to one score struct in one launch (nav_pop_test_summary), pbt_select ranks the members
and pairs the worst with the best, exploit() makes each of the worst a byte copy of its source's
learner in one launch (nav_td3_pop_exploit: networks, packed images, Adam moments, ring rows),
hands it the source's hyper-parameters and perturbs those named by `explore`; pbt_step() is the
three in a row. Nothing of it runs unless called.

Learning from the demonstrations per member: a member's overrides may carry demo_fraction,
bc_weight and q_weight (TD3Config; also bc_q_filter, the BC term's Q-filter, with
learner="members" only). Then every member's ring has a tail with the frame-0
transitions of its own env groups' demonstrations; learner="members" runs each TD3's one
epoch loop on its tailed ring, learner="batched" issues one nav_td3_mix_idx_pop per epoch and
nav_td3_actor_rows_bc_pop in place of nav_td3_actor_rows_pop, from a second device table of the
members' B_demo, tail sizes and weights. With the keys in no member's overrides nothing changes.

Resets to demonstration states per member: an override demo_reset_prob (not a field of either
struct) is the probability that an episode of the member's envs starts on a state of one of its
env group's demonstrations (VecEnv.set_demo_resets; one nav_demo_reset launch after the tick, the
members' values as its prob_group table, so members must own whole env groups). exploit() hands
it on like any other field and `explore` may perturb it; the table is rebuilt afterwards. With
the key in no member's overrides nothing is launched or allocated.
"""
import ctypes as C
import dataclasses
import itertools
import math

import numpy as np
import torch

from . import config as K
from ._lib import (NavMlp, NavParams, NavPopScore, NavReplay, NavTd3Member, NavTd3MemberBc,
                   NavTestOut, lib, params_struct, ptr, stream_handle)
from .demo_replay import DemoReplay
from .demos import demo_reset_usable
from .fields import make_field_device
from .td3 import TD3
from .trainer import episode_summary, make_env
from .vec_env import ReplayRing

PARAM_KEYS = frozenset(name for name, _ in NavParams._fields_)
# the learner's hyper-parameters a member may override (the batch size, the epoch count and the
# network shape belong to the whole population)
TD3_KEYS = frozenset(f.name for f in dataclasses.fields(K.TD3Config)) - {"batch_size",
                                                                         "num_epochs", "net"}
# neither struct: the member's starting exploration scale (robot.py:35 INITIAL_NOISE) and the
# seed of its learner (initial weights, replay sampling, target smoothing); and the env side's
# demo_reset_prob: the probability that an episode of the member's envs starts on a state of a
# demonstration (VecEnv.set_demo_resets; it reaches the kernel as prob_group)
EXTRA_KEYS = frozenset({"initial_noise", "seed", "demo_reset_prob"})
# population-based training. What a clone keeps of its own: its start values and its learner's
# seed; every other override it takes from its source
PBT_OWN_KEYS = frozenset({"initial_noise", "path_length0", "seed"})
# the float-valued per-member fields `explore` may perturb (what the population must share stays
# out: seeds, world_size, init_region_size, max_goal_draws, policy_update_delay, the batch size,
# the epoch count, the network shape)
PBT_PARAM_KEYS = frozenset({"demo_factor", "noise_decay", "stuck_penalty", "stuck_threshold",
                            "goal_reward", "goal_threshold", "max_action"})
# (bc_weight and q_weight weigh the actor's loss; demo_fraction stays out: it changes B_demo, the
# demonstration prefix of every batch)
PBT_TD3_KEYS = frozenset({"actor_lr", "critic_lr", "gamma", "tau", "policy_noise", "noise_clip",
                          "max_action", "bc_weight", "q_weight"})
# the env side's per-member floats, fields of neither struct
PBT_ENV_KEYS = frozenset({"demo_reset_prob"})
PBT_EXPLORE_KEYS = PBT_PARAM_KEYS | PBT_TD3_KEYS | PBT_ENV_KEYS
PBT_FACTORS = (0.8, 1.25)
# learning from the demonstrations, per member (TD3Config)
BC_KEYS = ("demo_fraction", "bc_weight", "q_weight")


def member_demo_groups(m, envs_per_member, envs_per_group, n_demos=K.NUM_DEMO):
    """Member m's env groups and their demonstrations in the CEM's group-major order: (range of
    groups, range of demonstrations, n_demos per group). A member's tail holds its own envs'
    demonstrations, so members must own whole groups."""
    epm, epg = int(envs_per_member), int(envs_per_group)
    if epg < 1 or epm % epg != 0:
        raise ValueError(f"members must own whole env groups: envs_per_member {epm} is not a "
                         f"multiple of envs_per_group {epg}")
    gpm = epm // epg
    groups = range(m * gpm, (m + 1) * gpm)
    return groups, range(groups.start * n_demos, groups.stop * n_demos)


def state_member(t, ring):
    """Learner t's state as a nav_td3_member: the six networks, the Adam moments and the replay
    ring; every other field stays null."""
    m = NavTd3Member()
    m.actor, m.target_actor = t.actor_network.desc(), t.target_actor.desc()
    m.critics[0], m.critics[1] = t.critic_network_1.desc(), t.critic_network_2.desc()
    m.target_critics[0] = t.target_critic_network_1.desc()
    m.target_critics[1] = t.target_critic_network_2.desc()
    m.replay = ring.desc()
    oa, oc1, oc2 = t.actor_optimizer, t.critic_optimizer_1, t.critic_optimizer_2
    m.m_actor, m.v_actor = oa.m.data_ptr(), oa.v.data_ptr()
    m.m_critic[0], m.m_critic[1] = oc1.m.data_ptr(), oc2.m.data_ptr()
    m.v_critic[0], m.v_critic[1] = oc1.v.data_ptr(), oc2.v.data_ptr()
    return m


def default_fitness(score):
    """Higher is better: the success rate, then the smaller mean best distance."""
    return (score["success_rate"], -score["mean_best_distance"])


def pbt_select(scores, frac=0.25, rng=None, fitness=None):
    """The (src, dst) lists of one exploit from the members' score dicts (scores()/evaluate()
    rows). Members are ranked best first by `fitness` (a score dict -> a sortable key, higher
    better; default (success_rate, -mean_best_distance)), ties to the lower member index. The
    k = floor(frac * P) worst (at least 1 for P >= 2, at most P // 2) are dst, worst first; the
    j-th worst takes the j-th best as src, or with `rng` (a numpy.random.Generator) the
    rng.integers(k)-th best. The two sets are disjoint, so the lists satisfy
    nav_td3_pop_exploit's rules. P = 1 gives no pairs."""
    P = len(scores)
    if P < 2:
        return [], []
    fit = fitness or default_fitness
    # a stable sort, reversed: equal keys keep the lower index first
    order = sorted(range(P), key=lambda m: fit(scores[m]), reverse=True)
    k = max(1, min(int(math.floor(frac * P)), P // 2))
    dst = order[::-1][:k]
    src = [order[j if rng is None else int(rng.integers(k))] for j in range(k)]
    return src, dst


def pbt_explore(values, explore, rng):
    """The explore rule on a clone's inherited values: for each name of `explore` (name ->
    (lo, hi)) the new value clip(values[name] * rng.choice([0.8, 1.25]), lo, hi). Returns the
    dict of new values; a name that is not an explorable per-member field raises KeyError."""
    out = {}
    for name, (lo, hi) in (explore or {}).items():
        if name not in PBT_EXPLORE_KEYS:
            raise KeyError(f"{name!r} cannot be explored: not one of the float-valued per-member "
                           f"fields {sorted(PBT_EXPLORE_KEYS)}")
        v = float(values[name]) * float(rng.choice(PBT_FACTORS))
        out[name] = min(max(v, float(lo)), float(hi))
    return out


def sweep_grid(**axes):
    """The cross product of the axes as a members list, the last axis varying fastest:
    sweep_grid(demo_factor=[10, 30], noise_decay=[0.5, 0.75]) -> 4 dicts of overrides."""
    names = list(axes)
    return [dict(zip(names, combo)) for combo in itertools.product(*(axes[k] for k in names))]


def route_overrides(overrides):
    """Split one member's overrides into (nav_params fields, TD3Config fields, extras). A key of
    both structs (max_action) goes to both. Unknown keys raise."""
    params, cfg, extra = {}, {}, {}
    for k, v in overrides.items():
        if k not in PARAM_KEYS | TD3_KEYS | EXTRA_KEYS:
            raise KeyError(f"unknown member override {k!r}: not a nav_params field "
                           f"({sorted(PARAM_KEYS)}), a TD3Config field ({sorted(TD3_KEYS)}) or "
                           f"one of {sorted(EXTRA_KEYS)}")
        if k in PARAM_KEYS:
            params[k] = v
        if k in TD3_KEYS:
            cfg[k] = v
        if k in EXTRA_KEYS:
            extra[k] = v
    return params, cfg, extra


class PopulationTable:
    """The host arrays and the device-resident member table of one population: member m's actor
    descriptor, `nav_params` and replay ring (rings None: test rollouts only). Built once on the
    stream (nav_pop_table_build); the launches read it, `replay_base` travels by value. The
    weights may change in place; call build() again after a descriptor's buffers, a constant or a
    ring changed."""

    def __init__(self, nets, params, rings, envs_per_member, stream=None):
        P = len(nets)
        assert P >= 1 and len(params) == P and (rings is None or len(rings) == P)
        self.nets, self.rings = list(nets), None if rings is None else list(rings)
        self.n_members, self.envs_per_member = P, int(envs_per_member)
        self.params = (NavParams * P)(*params)
        self.actors = (NavMlp * P)(*[n.desc() for n in nets])
        self.replays = None if rings is None else (NavReplay * P)(*[r.desc() for r in rings])
        nbytes = lib().nav_pop_table_bytes(P)
        self.table = torch.zeros(nbytes, dtype=torch.uint8, device=nets[0].device)
        self.build(stream)

    def build(self, stream=None):
        lib().nav_pop_table_build(self.params, self.actors, self.replays, self.n_members,
                                  self.envs_per_member, ptr(self.table), stream_handle(stream))


class PopulationLearner:
    """Every member's TD3 epoch (robot.py:258-285) in one launch per kernel. Built from the
    members' TD3 objects and rings; it owns no network: each TD3 stays the owner of its networks,
    moments and workspace (state_dict(), critic_loss_values() and checkpoints work per member as
    before), this class holds the device table of their kernel arguments and issues the launches.

    The members must agree on what the launches share: network shape, batch size,
    policy_update_delay, update_counter, the optimizers' step counts, betas and eps, and ring
    capacity and fill. Everything else (weights, seed, learning rates, gamma, tau, policy_noise,
    noise_clip, max_action, demo_fraction, bc_weight, q_weight) is the member's own. Call
    rebuild() after changing a member's hyper-parameter (cfg or an optimizer's lr) or replacing
    one of its buffers. If some member learns from demonstrations (TD3.bc_on), rebuild() also
    builds the BC table from the members' b_demo(), ring tails and weights, and update() runs
    TD3._update's demonstration steps for all members (mix_launches counts its mix launches, each
    member's _last_b_demo / bc_part serve its actor_loss_value() / bc_loss_value())."""

    def __init__(self, td3, rings, stream=None):
        self.td3, self.rings = list(td3), list(rings)
        P = self.P = len(self.td3)
        if P < 1 or len(self.rings) != P:
            raise ValueError("a population learner needs one ring per TD3, at least one")
        t0 = self.td3[0]
        for t in self.td3:
            if t.grad_hook is not None:
                raise ValueError("PopulationLearner: a TD3 with a grad_hook (shared policy) "
                                 "takes the per-member path")
            if (t.cfg.batch_size, t.cfg.net) != (t0.cfg.batch_size, t0.cfg.net):
                raise ValueError("PopulationLearner: one batch size and network shape")
        self._check_schedule()
        self.B = int(t0.cfg.batch_size)
        self.wgrad_splits = self.split_counts(P, t0.cfg.net.hidden, t0.cfg.net.n_hidden, self.B)
        # the twin online critics in separate workgroups: -1 = the library's choice from all
        # members' rows (1 / 0 force either form; the results are bit-identical)
        self.split_twins = -1
        self._inject = [(None, None, None)] * P
        self.table = torch.zeros(lib().nav_td3_pop_table_bytes(P), dtype=torch.uint8,
                                 device=t0.device)
        # learning from the demonstrations (a member's demo_fraction / bc_weight / q_weight): the
        # BC table and the members' nav_td3_member_bc array, built by rebuild() once some member
        # has it on (None: the epochs are the plain ones), and the mix launches issued
        self.bc_table = None
        self.bc_members = None
        self._mix = False
        self.mix_launches = 0
        self.rebuild(stream)

    @staticmethod
    def split_counts(n_members, hidden, n_hidden, batch):
        """(critic twins, actor) row splits of the weight-gradient launches that fill the chip
        with all members' tile jobs (nav_mlp_wgrad_splits_pop), as TD3's wgrad_splits= takes
        them."""
        hp = (int(hidden) + 31) // 32 * 32
        L = lib()
        sc = L.nav_mlp_wgrad_splits_pop(n_members, 2, 1, hp, n_hidden, batch)
        sa = L.nav_mlp_wgrad_splits_pop(n_members, 1, 2, hp, n_hidden, batch)
        return tuple(max(1, min(int(v), max(1, int(batch) // 32))) for v in (sc, sa))

    def _opts(self, t):
        return (t.critic_optimizer_1, t.critic_optimizer_2, t.actor_optimizer)

    def _check_schedule(self):
        t0 = self.td3[0]
        key = lambda t: (t.cfg.policy_update_delay, t.update_counter,  # noqa: E731
                         tuple((o.step_count, o.b1, o.b2, o.eps) for o in self._opts(t)))
        if any(key(t) != key(t0) for t in self.td3):
            raise ValueError("PopulationLearner: the members' policy_update_delay, update_counter "
                             "and optimizer step counts (and betas, eps) must be equal")
        c1, c2, _ = self._opts(t0)
        if (c1.step_count, c1.b1, c1.b2, c1.eps) != (c2.step_count, c2.b1, c2.b2, c2.eps):
            raise ValueError("PopulationLearner: the twin critics' optimizers must be in step")
        for t in self.td3:
            if t.critic_optimizer_1.lr != t.critic_optimizer_2.lr:
                raise ValueError("PopulationLearner: one learning rate for a member's twins")

    def inject(self, idx_critic=None, idx_actor=None, eps=None, stream=None):
        """Per member (lists of P tensors, or None): the critic batch's and the actor batch's
        sample indices (int64 [B]) and the target-smoothing noise (float32 [B][2]) that every
        later epoch uses instead of its Philox draws, as td3_update's idx_fn / eps_fn. The table
        holds the pointers: the tensors are kept alive here and may be refilled in place."""
        pick = lambda v, m: None if v is None else v[m]  # noqa: E731
        self._inject = [(pick(idx_critic, m), pick(idx_actor, m), pick(eps, m))
                        for m in range(self.P)]
        self.rebuild(stream)

    def _member(self, t, ring, inj):
        """state_member's fields, then the learner's hyper-parameters and workspace."""
        c = t.cfg
        m = state_member(t, ring)
        m.actor_lr, m.critic_lr = t.actor_optimizer.lr, t.critic_optimizer_1.lr
        m.policy_noise, m.noise_clip, m.max_action = c.policy_noise, c.noise_clip, c.max_action
        m.gamma, m.tau = c.gamma, c.tau
        m.seed_lo, m.seed_hi = t.seed & 0xFFFFFFFF, (t.seed >> 32) & 0xFFFFFFFF
        dp = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        m.idx_critic, m.idx_actor, m.eps = (dp(x) for x in inj)
        m.batch, m.batch_actor = t.batch.data_ptr(), t.batch2.data_ptr()
        for i, (dq, lp, es, ac, dz, mk, hs, g) in enumerate((
                (t.dq1, t.loss_part[0], t.eslab1, t.acts1, t.dz1, t.mask1, t.hslab, t.grad_c1),
                (t.dq2, t.loss_part[1], t.eslab2, t.acts2, t.dz2, t.mask2, t.hslab2, t.grad_c2))):
            m.dq[i], m.loss_part[i], m.edge_slabs[i] = dq.data_ptr(), lp.data_ptr(), es.data_ptr()
            m.acts[i], m.dz[i], m.masks[i] = ac.data_ptr(), dz.data_ptr(), mk.data_ptr()
            m.hidden_slabs[i], m.grad_critic[i] = hs.data_ptr(), g.data_ptr()
        m.edge_slabs_actor, m.acts_actor = t.eslab_a.data_ptr(), t.acts_a.data_ptr()
        m.dz_actor, m.masks_actor = t.dz_a.data_ptr(), t.mask_a.data_ptr()
        m.q, m.da, m.grad_actor = t.q1.data_ptr(), t.da.data_ptr(), t.grad_a.data_ptr()
        return m

    def rebuild(self, stream=None):
        """(Re)build the device table from the members' present buffers and hyper-parameters; each
        member's workspace is (re)allocated for the population's split counts first."""
        self._check_schedule()
        for t in self.td3:  # (a workspace that has them already stays)
            t.wgrad_splits = self.wgrad_splits
            t._workspace(self.B)
        inject, bc = self._inject, self._bc_members()
        if bc is not None:
            # every member's indices come from its idx_c / idx_a, which the mix launch fills; an
            # explicit inject() still wins (then for all members, and no mix is launched)
            given = [j[0] is not None or j[1] is not None for j in inject]
            self._mix = not any(given)
            if self._mix:
                inject = [(t.idx_c, t.idx_a, j[2]) for t, j in zip(self.td3, inject)]
            elif not all(j[0] is not None and j[1] is not None for j in inject):
                raise ValueError("PopulationLearner: with demonstration learning on, inject() "
                                 "takes both index arrays of every member or none")
            for b, j in zip(bc, inject):
                b.idx_critic, b.idx_actor = j[0].data_ptr(), j[1].data_ptr()
        self.members = (NavTd3Member * self.P)(*[
            self._member(t, r, j) for t, r, j in zip(self.td3, self.rings, inject)])
        lib().nav_td3_pop_table_build(self.members, self.P, self.B, self.wgrad_splits[0],
                                      self.wgrad_splits[1], ptr(self.table),
                                      stream_handle(stream))
        self.bc_members = None
        if bc is not None:
            self.bc_members = (NavTd3MemberBc * self.P)(*bc)
            if self.bc_table is None:
                self.bc_table = torch.zeros(lib().nav_td3_pop_bc_table_bytes(self.P),
                                            dtype=torch.uint8, device=self.td3[0].device)
            lib().nav_td3_pop_bc_table_build(self.members, self.bc_members, self.P, self.B,
                                             ptr(self.bc_table), stream_handle(stream))

    def _bc_members(self):
        """The members' nav_td3_member_bc entries (index pointers still unset), or None if no
        member learns from demonstrations. A member with it off takes B_demo = 0, bc_weight = 0
        and q_weight = 1: the plain actor loss, bit for bit."""
        for m, (t, ring) in enumerate(zip(self.td3, self.rings)):  # (built from bare TD3s too)
            t.cfg.check(population="batched", member=m)
            ring.check_serves(t.cfg)
        if not any(t.bc_on() for t in self.td3):
            return None
        out = []
        for t, ring in zip(self.td3, self.rings):
            b = NavTd3MemberBc()
            b.B_demo = t.b_demo() if t.bc_on() else 0
            b.n_demo = int(ring.tail.shape[0])
            b.q_weight, b.bc_weight = (t.cfg.q_weight, t.cfg.bc_weight) if t.bc_on() else (1.0, 0.0)
            b.bc_part = t.bc_part.data_ptr()
            out.append(b)
        return out

    def _step(self, group, soft_update, s):
        """The group's weight gradients, then reduce + Adam (+ the soft updates) and the packed
        images: every member's optimizer counts the step, the bias corrections (equal for all,
        _check_schedule) are the first one's (_Adam.bias_corrections)."""
        L = lib()
        L.nav_mlp_wgrad_pop(self.members, self.P, self.B, ptr(self.table), group,
                            self.wgrad_splits[group], s)
        o, *rest = [o for t in self.td3
                    for o in (self._opts(t)[:2] if group == 0 else self._opts(t)[2:])]
        for r in rest:
            r.step_count += 1
        bc1, bc2_sqrt = o.bias_corrections()
        L.nav_grad_reduce_adam_pop(self.members, self.P, self.B, ptr(self.table), group, o.b1,
                                   o.b2, o.eps, bc1, bc2_sqrt, int(soft_update), s)

    def update(self, num_epochs=None, stream=None):
        """TD3._update's epoch loop for every member at once, step for step: the policy-epoch
        test, the epoch's indices (with demonstrations one mix launch, the actor's on policy
        epochs only; injected ones come from the table), the critic rows and their step, then on
        a policy epoch the actor rows, plain or BC, and their step with the soft updates."""
        t0 = self.td3[0]
        n = t0.cfg.num_epochs if num_epochs is None else num_epochs
        size = len(self.rings[0])
        if any(len(r) != size for r in self.rings):
            raise ValueError("PopulationLearner: the rings must be filled alike")
        if size < 1:
            return
        c, L = t0.cfg, lib()
        bc = self.bc_members
        s, tab = stream_handle(stream), ptr(self.table)
        for epoch in range(n):
            policy = epoch % c.policy_update_delay == 0
            ctr = t0.update_counter
            if bc is not None and self._mix:
                self.mix_launches += 1
                L.nav_td3_mix_idx_pop(self.members, bc, self.P, self.B, ptr(self.bc_table), size,
                                      ctr, int(policy), s)
            L.nav_td3_critic_rows_pop(self.members, self.P, self.B, tab, size, ctr,
                                      self.split_twins, s)
            self._step(0, False, s)
            if policy:
                if bc is not None:
                    for t, b in zip(self.td3, bc):
                        t._last_b_demo = int(b.B_demo)
                    L.nav_td3_actor_rows_bc_pop(self.members, bc, self.P, self.B,
                                                ptr(self.bc_table), size, ctr, s)
                else:
                    L.nav_td3_actor_rows_pop(self.members, self.P, self.B, tab, size, ctr, s)
                self._step(1, True, s)
            for t in self.td3:
                t.update_counter += 1


class PopulationTrainer:
    """VecTrainer for P members at once. `members` is a list of dicts of overrides: fields of
    `nav_params` go to the member's constants (`path_length0` also fills the member's slice of
    path_length after init), fields of TD3Config to its learner, `initial_noise` fills its slice
    of noise_scale, `seed` seeds its learner and `demo_reset_prob` is the probability that an
    episode of its envs starts on a demonstration state. With one member and no overrides every
    step equals VecTrainer's with the same arguments, bit for bit."""

    def __init__(self, members, envs_per_member=4096, hidden=256, n_hidden=2, batch=4096,
                 updates_per_step=2, seed=K.RANDOM_SEED, envs_per_group=1024, demos=True,
                 streams=1, replay_capacity=None, device="cuda", field=None, learner="members",
                 wgrad_splits=None):
        self.members = [dict(m) for m in members]
        P = self.P = len(self.members)
        if P < 1:
            raise ValueError("a population needs at least one member")
        if not 1 <= int(streams) <= 4:
            raise ValueError("streams must be 1 .. 4")
        if learner not in ("members", "batched"):
            raise ValueError('learner must be "members" or "batched"')
        if learner == "batched" and int(streams) != 1:
            raise ValueError('learner="batched" issues one launch for all members: streams must '
                             'be 1')
        routed = [route_overrides(m) for m in self.members]
        if not demos and any(k in ck for _, ck, _ in routed for k in BC_KEYS):
            raise ValueError("demo_fraction / bc_weight / q_weight need demonstrations: "
                             "demos=True")
        # resets to demonstration states, per member (0 = off for the member)
        self.demo_reset_probs = [float(ex.get("demo_reset_prob", 0.0)) for _, _, ex in routed]
        for m, v in enumerate(self.demo_reset_probs):
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"demo_reset_prob must lie in [0, 1], got {v} (member {m})")
        if not demos and any(v > 0 for v in self.demo_reset_probs):
            raise ValueError("demo_reset_prob needs demonstrations: demos=True")
        # each member's config, and everything it refuses (the modes without a population form,
        # the BC term's Q-filter with the one-launch learner), before anything is built
        cfgs = [K.TD3Config(batch_size=int(batch), num_epochs=int(updates_per_step),
                            net=K.NetConfig(hidden=hidden, n_hidden=n_hidden), **ck)
                for _, ck, _ in routed]
        for m, cfg in enumerate(cfgs):
            cfg.check(population=learner, member=m)
        # learning from the demonstrations: on for a member whose demo_fraction or bc_weight is
        # non-zero (TD3.bc_on); then every member's ring carries a tail of its own envs'
        # demonstrations
        self.bc = any(cfg.bc_on() for cfg in cfgs)
        self.epm = int(envs_per_member)
        # members own whole env groups (ValueError otherwise)
        if self.bc or any(v > 0 for v in self.demo_reset_probs):
            member_demo_groups(0, self.epm, int(envs_per_group) if envs_per_group else self.epm)
        self.n = P * self.epm
        self.device = torch.device(device)
        self.seed = int(seed)
        if field is None:
            field = make_field_device(self.seed, self.device)
        self.field = field
        epg = int(envs_per_group) if envs_per_group else self.epm
        # (the CEM's states, actions and goals are kept for the members' DemoReplay)
        self.env, self._cem = make_env(self.n, field, self.seed, epg, demos, self.device)
        lo, hi = self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF
        self.params = [params_struct(seed_lo=lo, seed_hi=hi, **pk) for pk, _, _ in routed]
        cap = int(replay_capacity or max(4 * self.epm, 2 * int(batch), K.BUFFER_SIZE))
        # the members' rings, [P][cap][8]; with demonstration learning on [P][cap + tail][8]:
        # member m's tail holds the frame-0 transitions of its own env groups' demonstrations
        self.demo_replays = None
        tail = 0
        if self.bc:
            _, d0 = member_demo_groups(0, self.epm, epg)
            tail = len(d0) * (int(self._cem[0].shape[1]) - 1)
        self.ring_rows = torch.zeros(P, cap + tail, 8, dtype=torch.float32, device=self.device)
        self.rings = [ReplayRing(cap, self.device, rows=self.ring_rows[m], tail=tail)
                      for m in range(P)]
        if self.bc:
            self.demo_replays = [self._member_demos(m, self.rings[m]) for m in range(P)]
        self.td3 = []
        # the weight-gradient row splits: the batched learner's fill the chip with all members'
        # tiles; "members" takes TD3's own unless wgrad_splits= asks for others (to match a
        # batched run bit for bit)
        if learner == "batched":
            wgrad_splits = PopulationLearner.split_counts(P, hidden, n_hidden, int(batch))
        for m, ((pk, _, ex), cfg) in enumerate(zip(routed, cfgs)):
            t = TD3(cfg, device=self.device, seed=int(ex.get("seed", self.seed)),
                    wgrad_splits=wgrad_splits)
            t._workspace(cfg.batch_size)  # allocated now, on the stream every later one waits for
            self.td3.append(t)
            sl = self.member_slice(m)
            if "initial_noise" in ex:
                self.env.noise_scale[sl] = float(ex["initial_noise"])
            if "path_length0" in pk:
                self.env.path_length[sl] = int(pk["path_length0"])
        self.pop = PopulationTable([t.actor_network for t in self.td3], self.params, self.rings,
                                   self.epm)
        self._cem_host = None
        self._build_demo_resets()
        self.action = torch.zeros(self.n, 2, dtype=torch.float64, device=self.device)
        self.steps = 0
        self.updates_per_step = int(updates_per_step)
        self.streams = int(streams)
        self._side = None
        self.learner = PopulationLearner(self.td3, self.rings) if learner == "batched" else None
        # population-based training: the exploit events, the learner-state table
        # (nav_td3_pop_state_build, on first use), the scores' device buffer and the generator of
        # pbt_step's draws (seeded once from `seed`)
        self.pbt_history = []
        self._state = None
        self._score_buf = None
        self._pbt_rng = None

    def member_slice(self, m):
        return slice(m * self.epm, (m + 1) * self.epm)

    # ---- resets to demonstration states
    def _build_demo_resets(self):
        """The env's demo-reset set from the members' present values: each group takes its
        member's demo_reset_prob (prob_group) and each demonstration's usable count its member's
        goal_threshold. Nothing while no member has ever had a probability > 0."""
        if self.env._dreset is None and not any(v > 0 for v in self.demo_reset_probs):
            return
        if self._cem is None:
            raise ValueError("demo_reset_prob needs demonstrations: demos=True")
        st, _, goals = self._cem
        if self._cem_host is None:
            self._cem_host = st.cpu().numpy()
        usable, prob_group = [], []
        for m in range(self.P):
            g, d = member_demo_groups(m, self.epm, self.env.envs_per_group)
            usable.append(demo_reset_usable(self._cem_host[d.start:d.stop],
                                            goals[d.start:d.stop], self.params[m].goal_threshold))
            prob_group += [self.demo_reset_probs[m]] * len(g)
        self.env.set_demo_resets(st, np.concatenate(usable), 0.0, prob_group)

    def demo_reset_share(self, m):
        """VecEnv.demo_reset_share over member m's envs (whole 64-env rows). Synchronises."""
        if self.env.demo_resets is None:
            return 0.0
        sl = self.member_slice(m)
        taken = self.env.demo_resets[sl.start // 64:sl.stop // 64].sum().item()
        return float(taken) / float(self.env.episodes[sl].sum().item())

    # ---- learning from the demonstrations
    def _member_demos(self, m, ring=None):
        """Member m's DemoReplay: the transitions of its own env groups' demonstrations with its
        own constants, the frame-0 rows in `ring`'s tail if given."""
        if self._cem is None:
            raise ValueError("no demonstrations: construct with demos=True")
        st, ac, gl = self._cem
        _, d = member_demo_groups(m, self.epm, self.env.envs_per_group)
        sl = slice(d.start, d.stop)
        return DemoReplay(st[sl], ac[sl], gl[sl], self.params[m], ring=ring)

    def _demos(self, m):
        if self.demo_replays is None:
            self.demo_replays = [self._member_demos(k) for k in range(self.P)]
        return self.demo_replays[m]

    def pretrain_bc(self, epochs, lr=None, batch=None, stream=None):
        """VecTrainer.pretrain_bc member by member: each actor cloned on its own envs'
        demonstrations in the acting frame (start-up work, one member's launches after another's)."""
        for m, t in enumerate(self.td3):
            t.pretrain_bc(self._demos(m).rows1, epochs, batch, lr, stream)
        if self.learner is not None:
            self.learner.rebuild(stream)

    def bc_loss(self, frame=1):
        """Each member's BC loss over every row of its demonstrations in `frame`, in order."""
        return [t.bc_loss(self._demos(m).rows(frame)) for m, t in enumerate(self.td3)]

    def collect(self, stream=None):
        """Every member's action selection and tick: one launch."""
        self.env.act_tick_pop(self.pop, self.steps, self.rings[0].position,
                              action_out=self.action, stream=stream)
        for r in self.rings:
            r.advance(self.epm)
        self.steps += 1

    def _learn_member(self, m, stream):
        t = self.td3[m]
        if len(self.rings[m]) >= t.cfg.batch_size and self.updates_per_step > 0:
            t.td3_update(self.rings[m], self.updates_per_step, stream=stream)

    def learn(self, stream=None):
        """Each member's td3_update on its own ring. streams > 1: the members go round-robin over
        that many side streams, which start after the tick and are joined before this returns
        control of `stream` (the members share nothing, so the results do not depend on it).
        learner="batched": every member's epochs in one launch per kernel (PopulationLearner),
        once every ring holds a batch."""
        if self.learner is not None:
            if (self.updates_per_step > 0 and
                    all(len(r) >= self.learner.B for r in self.rings)):
                self.learner.update(self.updates_per_step, stream)
            return
        if self.streams == 1:
            for m in range(self.P):
                self._learn_member(m, stream)
            return
        main = stream if stream is not None else torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = [torch.cuda.Stream(self.device) for _ in range(self.streams)]
            self._ticked = torch.cuda.Event()
            self._done = [torch.cuda.Event() for _ in range(self.streams)]
        self._ticked.record(main)
        for s in self._side:
            s.wait_event(self._ticked)
        for m in range(self.P):
            self._learn_member(m, self._side[m % self.streams])
        for s, e in zip(self._side, self._done):
            e.record(s)
            main.wait_event(e)

    def step(self, stream=None):
        self.collect(stream)
        self.learn(stream)

    def evaluate(self, max_steps=K.TEST_TIMEOUT * K.UPDATE_RATE, episode=0, start=None):
        """One greedy test episode per env with its member's online actor, max_action and
        goal_threshold, all members in one launch; per member the dict of VecTrainer.evaluate()
        over its envs plus its overrides. Training state is untouched."""
        out = self.env.test_rollout_pop(self.pop, max_steps, episode=episode, start=start)
        res = []
        for m in range(self.P):
            sl = self.member_slice(m)
            d = episode_summary(out["reached"][sl], out["steps"][sl], out["best_distance"][sl],
                                max_steps, episode)
            d.update(self.members[m])
            res.append(d)
        return res

    # ---- population-based training
    def scores(self, max_steps=K.TEST_TIMEOUT * K.UPDATE_RATE, episode=0, start=None,
               stream=None):
        """evaluate()'s rows from one rollout launch, one reduction launch
        (nav_pop_test_summary: fixed-order sums per member) and one device-to-host copy of the
        [P] score structs, instead of four or five synchronising reductions per member. The
        sums run in another order than torch's, so mean_best_distance may differ from
        evaluate()'s in the last bits; the counts and the maximum are equal."""
        out = self.env.test_rollout_pop(self.pop, max_steps, episode=episode, start=start,
                                        stream=stream)
        if self._score_buf is None:
            self._score_buf = torch.zeros(self.P * C.sizeof(NavPopScore), dtype=torch.uint8,
                                          device=self.device)
        o = NavTestOut(ptr(out["reached"]), ptr(out["steps"]), ptr(out["best_distance"]), None,
                       None)
        lib().nav_pop_test_summary(C.byref(o), self.P, self.epm, ptr(self._score_buf),
                                   stream_handle(stream))
        if stream is not None:
            stream.synchronize()
        host = (NavPopScore * self.P).from_buffer_copy(self._score_buf.cpu().numpy().tobytes())
        res = []
        for m, s in enumerate(host):
            d = {"n": self.epm,
                 "reached": int(s.reached),
                 "success_rate": s.reached / self.epm,
                 "mean_steps_reached": (s.steps_reached / s.reached if s.reached
                                        else float("nan")),
                 "mean_best_distance": s.sum_best / self.epm,
                 "max_best_distance": s.max_best,
                 "max_steps": int(max_steps),
                 "episode": int(episode)}
            d.update(self.members[m])
            res.append(d)
        return res

    def state_table(self, stream=None, rebuild=False):
        """(the nav_td3_member array, the device table) of the members' learner state, built on
        first use and kept: the networks, moments and rings change in place. rebuild=True after
        a buffer was replaced."""
        if self._state is None or rebuild:
            # (nav_td3_pop_exploit neither reads nor writes what state_member leaves null)
            arr = (NavTd3Member * self.P)(*[state_member(t, r)
                                            for t, r in zip(self.td3, self.rings)])
            tab = torch.zeros(lib().nav_td3_pop_state_bytes(self.P), dtype=torch.uint8,
                              device=self.device)
            lib().nav_td3_pop_state_build(arr, self.P, ptr(tab), stream_handle(stream))
            self._state = (arr, tab)
        return self._state

    def member_value(self, m, key):
        """Member m's present value of a per-member field: the learner's for a TD3Config field,
        else the nav_params field."""
        if key in PBT_ENV_KEYS:
            return self.demo_reset_probs[m]
        if key in TD3_KEYS:
            return getattr(self.td3[m].cfg, key)
        return getattr(self.params[m], key)

    def _set_member_value(self, m, key, value):
        if key in PBT_ENV_KEYS:
            self.demo_reset_probs[m] = float(value)
        if key in PARAM_KEYS:
            setattr(self.params[m], key, value)
        if key in TD3_KEYS:
            t = self.td3[m]
            setattr(t.cfg, key, value)
            if key == "actor_lr":
                t.actor_optimizer.lr = value
            if key == "critic_lr":
                t.critic_optimizer_1.lr = t.critic_optimizer_2.lr = value

    def exploit(self, src, dst, copy_replay=True, explore=None, rng=None, stream=None):
        """Member dst[j] becomes a continuation of member src[j]: its six networks, their packed
        images, the six Adam moments and (copy_replay) the filled rows of the ring are copied in
        one launch (nav_td3_pop_exploit), then the host's books follow. dst keeps its learner's
        seed, its envs and their state and its start values (initial_noise, path_length0); it
        takes src's value of every other per-member field, then `explore` (name -> (lo, hi))
        perturbs the named ones: clip(value * rng.choice([0.8, 1.25]), lo, hi). The new values go
        to members[dst], params[dst], td3[dst].cfg and the optimizers' lr; the member table (and
        the batched learner's) is rebuilt. Appends one event per pair to pbt_history."""
        src, dst = [int(s) for s in src], [int(d) for d in dst]
        if len(src) != len(dst):
            raise ValueError("exploit: one src per dst")
        for name in (explore or {}):  # before anything is copied
            if name not in PBT_EXPLORE_KEYS:
                raise KeyError(f"{name!r} cannot be explored: not one of the float-valued "
                               f"per-member fields {sorted(PBT_EXPLORE_KEYS)}")
        # a clone without demonstration rows in its batches keeps bc_weight 0 (a source's own is 0
        # then, so only a lower bound above 0 could lift it): refused as TD3.b_demo refuses it
        if explore and float(explore.get("bc_weight", (0.0, 0.0))[0]) > 0:
            for s in src:
                dataclasses.replace(self.td3[s].cfg, bc_weight=1.0).check(member=s)
        # a lower bound above 0 can switch resets on for a population built without them: then
        # the demonstrations and the whole-groups rule are needed, as at construction
        if explore and float(explore.get("demo_reset_prob", (0.0, 0.0))[0]) > 0:
            if self._cem is None:
                raise ValueError("demo_reset_prob needs demonstrations: demos=True")
            member_demo_groups(0, self.epm, self.env.envs_per_group)
        if not src:
            return []
        if explore and rng is None:
            rng = self.pbt_rng()
        arr, tab = self.state_table(stream)
        n = len(src)
        rows = len(self.rings[src[0]]) if copy_replay else 0
        lib().nav_td3_pop_exploit(arr, self.P, ptr(tab), (C.c_int32 * n)(*src),
                                  (C.c_int32 * n)(*dst), n, rows, stream_handle(stream))
        # every per-member field but the clone's own: the members' overrides name only some
        inherited = sorted((PARAM_KEYS | TD3_KEYS | PBT_ENV_KEYS) - PBT_OWN_KEYS
                           - {"seed_lo", "seed_hi"})
        events = []
        for s, d in zip(src, dst):
            before = {k: self.member_value(d, k) for k in inherited}
            values = {k: self.member_value(s, k) for k in inherited}
            values.update(pbt_explore(values, explore, rng))
            for k, v in values.items():
                self._set_member_value(d, k, v)
            own = {k: v for k, v in self.members[d].items() if k in PBT_OWN_KEYS}
            taken = {k: values[k] for k in self.members[s] if k not in PBT_OWN_KEYS}
            taken.update({k: values[k] for k in (explore or {})})
            self.members[d] = {**own, **taken}
            if copy_replay:
                self.rings[d].position, self.rings[d].size = (self.rings[s].position,
                                                              self.rings[s].size)
            changed = {k: (before[k], values[k]) for k in inherited if before[k] != values[k]}
            events.append({"step": self.steps, "src": s, "dst": d, "replay_rows": rows,
                           "before": {k: b for k, (b, _) in changed.items()},
                           "after": {k: a for k, (_, a) in changed.items()},
                           "explored": {k: values[k] for k in (explore or {})}})
            self.pop.params[d] = self.params[d]
        self.pop.build(stream)
        self._build_demo_resets()  # the groups' probabilities (prob_group) follow the members
        if self.learner is not None:
            self.learner.rebuild(stream)
        self.pbt_history.extend(events)
        return events

    def pbt_rng(self):
        """The generator of pbt_step's draws, seeded once from the trainer's seed."""
        if self._pbt_rng is None:
            self._pbt_rng = np.random.default_rng(self.seed)
        return self._pbt_rng

    def pbt_step(self, frac=0.25, explore=None, rng=None, copy_replay=True,
                 max_steps=K.TEST_TIMEOUT * K.UPDATE_RATE, fitness=None, stream=None):
        """One step of population-based training: scores(), pbt_select, exploit. Returns the
        scores and the (src, dst) pairs. rng=None draws from pbt_rng(), so a run repeats."""
        rng = self.pbt_rng() if rng is None else rng
        sc = self.scores(max_steps=max_steps, stream=stream)
        src, dst = pbt_select(sc, frac=frac, rng=rng, fitness=fitness)
        self.exploit(src, dst, copy_replay=copy_replay, explore=explore, rng=rng, stream=stream)
        return sc, (src, dst)

    def env_steps(self):
        return self.steps * self.n
