"""Population training: P members, each with its own actor, twin critics and learner, its own
replay ring and its own `nav_params`, on ONE env set, acting and ticking in ONE launch and running
their test episodes in ONE launch (nav_act_tick_pop / nav_test_rollout_pop).

The reference's only published result is a hyper-parameter study (the score over
DEMO_PROXIMITY_FACTOR in {10, 30, 50, 70}; simulator.py:169-200 attempts the same over
INITIAL_NOISE x NOISE_DECAY). Envs are independent of each other (environment.py:98-137), so a
sweep is a population: member m owns the consecutive envs [m * envs_per_member, (m + 1) *
envs_per_member) and ends exactly as it would alone on the whole env set, bit for bit. The
learner's row kernels are not batched over members: each member's td3_update runs today's kernels
at its batch size, optionally round-robin over a few streams.
"""
import ctypes as C
import dataclasses
import itertools

import torch

from . import config as K
from ._lib import NavMlp, NavParams, NavReplay, lib, params_struct, ptr, stream_handle
from .cem import cem_group_demo_sets
from .fields import make_field_device
from .td3 import TD3
from .vec_env import ReplayRing, VecEnv

PARAM_KEYS = frozenset(name for name, _ in NavParams._fields_)
# the learner's hyper-parameters a member may override (the batch size, the epoch count and the
# network shape belong to the whole population)
TD3_KEYS = frozenset(f.name for f in dataclasses.fields(K.TD3Config)) - {"batch_size",
                                                                         "num_epochs", "net"}
# neither struct: the member's starting exploration scale (robot.py:35 INITIAL_NOISE) and the
# seed of its learner (initial weights, replay sampling, target smoothing)
EXTRA_KEYS = frozenset({"initial_noise", "seed"})


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


class PopulationTrainer:
    """VecTrainer for P members at once. `members` is a list of dicts of overrides: fields of
    `nav_params` go to the member's constants (`path_length0` also fills the member's slice of
    path_length after init), fields of TD3Config to its learner, `initial_noise` fills its slice
    of noise_scale and `seed` seeds its learner. With one member and no overrides every step
    equals VecTrainer's with the same arguments, bit for bit."""

    def __init__(self, members, envs_per_member=4096, hidden=256, n_hidden=2, batch=4096,
                 updates_per_step=2, seed=K.RANDOM_SEED, envs_per_group=1024, demos=True,
                 streams=1, replay_capacity=None, device="cuda", field=None):
        self.members = [dict(m) for m in members]
        P = self.P = len(self.members)
        if P < 1:
            raise ValueError("a population needs at least one member")
        if not 1 <= int(streams) <= 4:
            raise ValueError("streams must be 1 .. 4")
        routed = [route_overrides(m) for m in self.members]
        self.epm = int(envs_per_member)
        self.n = P * self.epm
        self.device = torch.device(device)
        self.seed = int(seed)
        if field is None:
            field = make_field_device(self.seed, self.device)
        self.field = field
        epg = int(envs_per_group) if envs_per_group else self.epm
        self.env = VecEnv(self.n, field, seed=self.seed, envs_per_group=epg, demo_flag=demos,
                          device=self.device)
        if demos:  # as VecTrainer: each group's demonstrations from the batched CEM
            G = (self.n + epg - 1) // epg
            firsts = torch.arange(G, device=self.device) * epg
            pts, off = cem_group_demo_sets(self.field, self.env.region[firsts].cpu().numpy(),
                                           self.env.goal[firsts].cpu().numpy(), self.seed,
                                           device=self.device)
            self.env.set_demo(pts, off if G > 1 else None)
        lo, hi = self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF
        self.params = [params_struct(seed_lo=lo, seed_hi=hi, **pk) for pk, _, _ in routed]
        cap = int(replay_capacity or max(4 * self.epm, 2 * int(batch), K.BUFFER_SIZE))
        self.ring_rows = torch.zeros(P, cap, 8, dtype=torch.float32, device=self.device)
        self.rings = [ReplayRing(cap, self.device, rows=self.ring_rows[m]) for m in range(P)]
        self.td3 = []
        for m, (pk, ck, ex) in enumerate(routed):
            cfg = K.TD3Config(batch_size=int(batch), num_epochs=int(updates_per_step),
                              net=K.NetConfig(hidden=hidden, n_hidden=n_hidden), **ck)
            t = TD3(cfg, device=self.device, seed=int(ex.get("seed", self.seed)))
            t._workspace(cfg.batch_size)  # allocated now, on the stream every later one waits for
            self.td3.append(t)
            sl = self.member_slice(m)
            if "initial_noise" in ex:
                self.env.noise_scale[sl] = float(ex["initial_noise"])
            if "path_length0" in pk:
                self.env.path_length[sl] = int(pk["path_length0"])
        self.pop = PopulationTable([t.actor_network for t in self.td3], self.params, self.rings,
                                   self.epm)
        self.action = torch.zeros(self.n, 2, dtype=torch.float64, device=self.device)
        self.steps = 0
        self.updates_per_step = int(updates_per_step)
        self.streams = int(streams)
        self._side = None

    def member_slice(self, m):
        return slice(m * self.epm, (m + 1) * self.epm)

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
        control of `stream` (the members share nothing, so the results do not depend on it)."""
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
            reached = out["reached"][sl].bool()
            n_reached = int(reached.sum().item())
            best = out["best_distance"][sl]
            d = {"n": self.epm,
                 "success_rate": out["reached"][sl].float().mean().item(),
                 "mean_steps_reached": (out["steps"][sl][reached].double().mean().item()
                                        if n_reached else float("nan")),
                 "mean_best_distance": best.mean().item(),
                 "max_best_distance": best.max().item(),
                 "max_steps": int(max_steps),
                 "episode": int(episode)}
            d.update(self.members[m])
            res.append(d)
        return res

    def env_steps(self):
        return self.steps * self.n
