"""Vectorised residual-TD3 training loop on one GPU (the MI355X form of robot-learning.py's
training mode, robot-learning.py:54-101, for n independent envs at once).

One `step()` = one vector tick: every env selects an action (actor MLP + baseline + exploration
noise) and takes one environment step with the fused reward / stuck / done / replay-push /
auto-reset tick, both in ONE launch (nav_act_tick), then the learner runs `updates_per_step`
TD3 epochs (robot.py:272-285: critic every epoch, actor + Polyak every `policy_update_delay`-th)
on batches sampled from the device replay ring. The reference's schedule (100 epochs of batch
100 at every episode end) does not map onto 65 536 asynchronous envs; the update-to-data ratio
here is updates_per_step * batch / n_envs sampled transitions per collected transition.
"""
import ctypes as C

import numpy as np
import torch

from . import config as K
from . import prof
from ._lib import lib, ptr, stream_handle
from .cem import cem_group_demo_sets
from .demo_replay import DemoReplay
from .demos import demo_reset_usable
from .fields import make_field_device
from .td3 import TD3
from .vec_env import ReplayRing, VecEnv, ring_needs


def make_env(n, field, seed, envs_per_group, demos, device):
    """The VecEnv of n envs and, with `demos`, its demo set: each group's 3 demonstrations from
    the batched GPU CEM (environment.py:140-179) + their augmentations (robot.py:771-824), as the
    reference's robot acquires them. -> (env, the CEM's [states, actions, goals], kept for the
    DemoReplay; None without demos)."""
    epg = int(envs_per_group)
    env = VecEnv(n, field, seed=seed, envs_per_group=epg, demo_flag=demos, device=device)
    if not demos:
        return env, None
    G = (n + epg - 1) // epg
    firsts = torch.arange(G, device=device) * epg
    pts, off, *cem = cem_group_demo_sets(field, env.region[firsts].cpu().numpy(),
                                         env.goal[firsts].cpu().numpy(), seed, device=device,
                                         with_transitions=True)
    env.set_demo(pts, off if G > 1 else None)
    return env, cem


def episode_summary(reached, steps, best_distance, max_steps, episode):
    """The summary of one test episode per env (test_rollout's outputs, or a member's slice of
    them) as a plain dict."""
    hit = reached.bool()
    n_reached = int(hit.sum().item())
    return {"n": int(reached.shape[0]),
            "success_rate": reached.float().mean().item(),
            "mean_steps_reached": (steps[hit].double().mean().item() if n_reached
                                   else float("nan")),
            "mean_best_distance": best_distance.mean().item(),
            "max_best_distance": best_distance.max().item(),
            "max_steps": int(max_steps),
            "episode": int(episode)}


class VecTrainer:
    def __init__(self, n_envs=65536, hidden=256, n_hidden=2, batch=32768, updates_per_step=2,
                 replay_capacity=None, seed=K.RANDOM_SEED, envs_per_group=1024, demos=True,
                 device="cuda", field=None, grad_hook=None, fuse_tick=True, overlap_collect=False,
                 demo_rows=None, demo_reset_prob=0.0, **modes):
        """**modes: the learner's mode fields (config.MODE_FIELDS; any other keyword is a
        TypeError), each at TD3Config's default; what does not combine is TD3Config.check's.
        demo_fraction / bc_weight / q_weight: learning from the demonstrations (TD3Config; off
        by default). With demo_fraction or bc_weight non-zero the CEM demonstrations' transitions
        sit in a tail behind the replay ring and a share of every batch is drawn from it (needs
        demos=True, or demo_rows = (frame-0 rows, frame-1 rows) from a checkpoint).
        bc_q_filter: the Q-filter of the BC term (TD3Config; off by default): a demonstration row
        is cloned only where critic 1 rates its action above the policy's;
        td3.bc_kept_fraction() reports the share of rows the last policy epoch kept.
        per_alpha / per_beta / per_eps: prioritised replay (TD3Config; off at per_alpha == 0).
        On, the ring carries one priority per row, every tick stamps its rows with the running
        maximum, and batches are drawn in proportion to priority.
        n_step: multi-step returns (TD3Config; off at 1). On, the ring carries one cut mark per
        row, every tick writes its rows' marks from its flags, and the critics' target sums up to
        n_step rewards along the env's rows (stride n_envs).
        demo_reset_prob: resets to demonstration states (Nair et al. 2018; an env-side feature,
        not a learner mode; off at 0). An episode then starts with this probability on a state of
        one of its env group's CEM demonstrations instead of the init-region draw (one
        nav_demo_reset launch after every tick; needs demos=True); env.demo_reset_share()
        reports the share. evaluate()'s test episodes still start in the init regions."""
        for k in modes:
            if k not in K.MODE_FIELDS:
                raise TypeError(f"VecTrainer() got an unexpected keyword argument {k!r}")
        # the learner's config, and everything it refuses, before anything is built
        cfg = K.TD3Config(batch_size=int(batch), num_epochs=int(updates_per_step),
                          net=K.NetConfig(hidden=hidden, n_hidden=n_hidden),
                          **K.mode_kwargs(modes))
        cfg.check(grad_hook, overlap_collect)
        need = ring_needs(cfg)
        if need["tail"] and not demos and demo_rows is None:
            raise ValueError("demo_fraction / bc_weight need demonstrations: demos=True")
        self.demo_reset_prob = float(demo_reset_prob)
        if not 0.0 <= self.demo_reset_prob <= 1.0:
            raise ValueError(f"demo_reset_prob must lie in [0, 1], got {demo_reset_prob}")
        if self.demo_reset_prob > 0 and not demos:
            raise ValueError("demo_reset_prob needs demonstrations: demos=True")
        self.n = int(n_envs)
        self.device = torch.device(device)
        self.seed = int(seed)
        if field is None:  # set_dynamics on the device (nav_fields_generate)
            field = make_field_device(self.seed, self.device)
        self.field = field
        self.env, self._cem = make_env(self.n, field, self.seed, envs_per_group or self.n, demos,
                                       self.device)
        if self.demo_reset_prob > 0:  # the CEM's states and, per demonstration, its goal
            st, _, goals = self._cem
            self.env.set_demo_resets(st, demo_reset_usable(st.cpu().numpy(), goals,
                                                           self.env.p.goal_threshold),
                                     self.demo_reset_prob)
        self.td3 = TD3(cfg, device=self.device, seed=self.seed, grad_hook=grad_hook)
        cap = replay_capacity or max(4 * self.n, 2 * int(batch), K.BUFFER_SIZE)
        # the ring the config needs. The demonstration transitions: in its tail when the learner
        # draws from them, else built on the first pretrain_bc / bc_loss (the ring is what it was)
        tail = 0
        if need["tail"]:  # a checkpoint's rows, else every transition of the CEM's demonstrations
            st = self._cem[0] if demo_rows is None else None
            tail = demo_rows[0].shape[0] if st is None else st.shape[0] * (st.shape[1] - 1)
        self.replay = ReplayRing(cap, self.device, tail=tail, priorities=need["priorities"],
                                 cuts=need["cuts"])
        ring = self.replay if need["tail"] else None
        self.demo_replay = None
        if demo_rows is not None:
            self.demo_replay = DemoReplay.from_rows(demo_rows[0].to(self.device), demo_rows[1],
                                                    ring)
        elif ring is not None:
            self.demo_replay = DemoReplay(*self._cem, self.env.p, ring=ring)
        self.replay.stride = self.n  # an env's next transition: n_envs rows on
        self.action = torch.zeros(self.n, 2, dtype=torch.float64, device=self.device)
        self.steps = 0
        self.updates_per_step = int(updates_per_step)
        # act + tick fused into one launch (False: the two launches; A/B and the fused-vs-unfused
        # parity test)
        self.fuse_tick = bool(fuse_tick)
        # shared policy: the next step's collect on a second stream beside the last epoch's
        # critic all-reduce and Adam step (bit-identical either way). Off by default: the two
        # cross-stream waits per step cost ~24 us on one MI355X (profiles/r05u_shared_policy_host
        # .json), so it pays only where the collective itself takes longer than that.
        self.overlap_collect = bool(overlap_collect)
        self._side = None
        self._collect_ready = None  # recorded by the last learn() (td3_update collect_ready)
        self._collected = None

    # robot.py:541-569 for every env
    def act(self, training=True, stream=None):
        net = self.td3.actor_network
        a = net.desc()
        with prof.region("act", prof.mlp_fwd_flops(2, 2, net.hidden, net.n_hidden, self.n)):
            lib().nav_act(C.byref(self.env.p), C.byref(a), self.n, ptr(self.env.state),
                          ptr(self.env.goal), ptr(self.env.noise_scale), None, self.steps,
                          0 if training else 1, ptr(self.action), None, stream_handle(stream))
        return self.action

    def collect(self, stream=None):
        if self.fuse_tick and (self.env.demo_xy is None or self.env.demo_index is not None):
            # one launch: action selection + the tick (nav_act_tick)
            self.env.act_tick(self.td3.actor_network, self.steps, self.replay,
                              action_out=self.action, stream=stream)
        else:
            self.act(True, stream)
            self.env.agent_step(self.action, self.replay, stream)
        self.steps += 1

    def learn(self, stream=None, collect_ready=None):
        if len(self.replay) >= self.td3.cfg.batch_size and self.updates_per_step > 0:
            self.td3.td3_update(self.replay, self.updates_per_step, stream=stream,
                                collect_ready=collect_ready)
        elif collect_ready is not None:
            collect_ready.record(stream)

    def step(self, stream=None):
        if not self.overlap_collect or prof._active is not None:
            self.sync_collect()
            self.collect(stream)
            self.learn(stream)
            return
        # overlapped form (shared policy): this collect reads only the actor and the env state
        # and writes the env state and the replay ring, so it may start once the previous learn
        # has issued its last replay read and actor write (td3_update's collect_ready: before
        # the final critic-only epoch's all-reduce); the learn waits for the collect
        main = stream if stream is not None else torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
            self._collected = torch.cuda.Event()
        side = self._side
        if self._collect_ready is None:
            side.wait_stream(main)
        else:
            side.wait_event(self._collect_ready)
        self.collect(side)
        self._collected.record(side)
        main.wait_event(self._collected)
        if self._collect_ready is None:
            self._collect_ready = torch.cuda.Event()
        self.learn(main, self._collect_ready)

    def sync_collect(self):
        """Make the next step's collect wait for everything issued on the current stream (after
        host-side changes to the env state, the replay ring or the actor between steps)."""
        self._collect_ready = None

    # robot-learning.py's testing mode (78, 104-117) over all envs with the online actor
    def evaluate(self, max_steps=K.TEST_TIMEOUT * K.UPDATE_RATE, episode=0, start=None):
        """One greedy test episode per env (VecEnv.test_rollout) and its summary as a plain dict.
        Reads the online actor, the goals and the init regions only: the env state, the replay
        ring, the step counter and the learner are untouched."""
        out = self.env.test_rollout(self.td3.actor_network, max_steps, episode=episode,
                                    start=start)
        return episode_summary(out["reached"], out["steps"], out["best_distance"], max_steps,
                               episode)

    # ---- the imitation baseline (the reference README's "baseline policy by imitation")
    def _demos(self):
        if self.demo_replay is None:
            if self._cem is None:
                raise ValueError("no demonstrations: construct with demos=True")
            self.demo_replay = DemoReplay(*self._cem, self.env.p)
        return self.demo_replay

    def pretrain_bc(self, epochs, batch=None, lr=None, stream=None):
        """Pure behaviour cloning of the actor on the demonstrations in the acting frame
        (TD3.pretrain_bc on the frame-1 rows), before any environment step: afterwards evaluate()
        scores baseline + actor(s - g) as an imitation of the demonstrated actions."""
        self.td3.pretrain_bc(self._demos().rows1, epochs, batch, lr, stream)
        self.sync_collect()

    def bc_loss(self, frame=1):
        """The actor's BC loss over every demonstration row of `frame`, in order."""
        return self.td3.bc_loss(self._demos().rows(frame))

    def env_steps(self):
        return self.steps * self.n

    # ---- checkpoint / resume: every piece of state the next step reads
    ENV_STATE = ("state", "goal", "region", "hist", "meta", "plan_index", "path_length",
                 "episodes", "noise_scale")

    def state_dict(self):
        """The trainer's whole state as host tensors and plain values (torch.save-able, loadable
        with weights_only=True): per-env SoA state, field, demo set, replay ring, learner (nets,
        Adam moments, counters) and the step counter that keys the exploration noise. A trainer
        restored from it continues bit for bit as the original would have."""
        e = self.env
        sd = {
            "meta": {"n_envs": self.n, "seed": self.seed, "envs_per_group": e.envs_per_group,
                     "hidden": self.td3.actor_network.hidden,
                     "n_hidden": self.td3.actor_network.n_hidden,
                     "batch": self.td3.cfg.batch_size, "updates_per_step": self.updates_per_step,
                     "steps": self.steps, **K.mode_meta(self.td3.cfg)},
            "demo_rows": None if self.demo_replay is None else
            {"rows0": self.demo_replay.rows0.cpu(), "rows1": self.demo_replay.rows1.cpu()},
            "env": {k: getattr(e, k).detach().cpu() for k in self.ENV_STATE},
            "field": self.field.detach().cpu(),
            "demo_xy": None if e.demo_xy is None else e.demo_xy.cpu(),
            "demo_off": None if e.demo_off is None else e.demo_off.cpu(),
            "replay": {"rows": self.replay.rows.cpu(), "position": self.replay.position,
                       "size": self.replay.size},
            "td3": self.td3.state_dict(),
        }
        if self.td3.per_on():  # prioritised replay: the priority store
            sd["replay"].update(pri=self.replay.pri.cpu(), stat=self.replay.stat.cpu())
        if self.td3.nstep_on():  # multi-step returns: the cut marks
            sd["replay"].update(cut=self.replay.cut.cpu())
        if self.demo_reset_prob > 0:  # resets to demonstration states: the set and the counts
            d = e._dreset
            sd["demo_reset"] = {"prob": self.demo_reset_prob, "states": d["states"].cpu(),
                                "usable": d["usable"].cpu(), "counts": e.demo_resets.cpu()}
        return sd

    def load_state_dict(self, sd):
        m = sd["meta"]
        assert (m["n_envs"], m["envs_per_group"]) == (self.n, self.env.envs_per_group)
        assert sd["replay"]["rows"].shape == self.replay.rows.shape
        for k in self.ENV_STATE:
            getattr(self.env, k).copy_(sd["env"][k].to(self.device))
        self.field.copy_(sd["field"].to(self.device))
        if sd["demo_xy"] is not None:
            self.env.set_demo(sd["demo_xy"], sd["demo_off"])
        self.replay.rows.copy_(sd["replay"]["rows"].to(self.device))
        self.replay.position = int(sd["replay"]["position"])
        self.replay.size = int(sd["replay"]["size"])
        if self.td3.per_on():
            self.replay.pri.copy_(sd["replay"]["pri"].to(self.device))
            self.replay.stat.copy_(sd["replay"]["stat"].to(self.device))
            self.td3.cfg.per_beta = float(m["per_beta"])
        if self.td3.nstep_on():
            self.replay.cut.copy_(sd["replay"]["cut"].to(self.device))
        dr = sd.get("demo_reset")  # absent in a checkpoint written with the feature off
        if dr is not None:
            self.demo_reset_prob = float(dr["prob"])
            self.env.set_demo_resets(dr["states"], dr["usable"], self.demo_reset_prob)
            self.env.demo_resets.copy_(dr["counts"].to(self.device))
        self.td3.load_state_dict(sd["td3"])
        self.steps = int(m["steps"])
        self.updates_per_step = int(m["updates_per_step"])
        self.sync_collect()

    @classmethod
    def from_state_dict(cls, sd, device="cuda", grad_hook=None):
        """A trainer resumed from state_dict() without re-running the field generator or the CEM
        (their results are in the checkpoint)."""
        m = sd["meta"]
        dr = sd.get("demo_rows")
        t = cls(n_envs=m["n_envs"], hidden=m["hidden"], n_hidden=m["n_hidden"],
                batch=m["batch"], updates_per_step=m["updates_per_step"],
                replay_capacity=sd["replay"]["rows"].shape[0], seed=m["seed"],
                envs_per_group=m["envs_per_group"], demos=False, device=device,
                field=sd["field"].to(device), grad_hook=grad_hook,
                demo_rows=None if dr is None else (dr["rows0"], dr["rows1"]),
                **K.mode_kwargs(m))
        t.load_state_dict(sd)
        return t

    def save(self, path):
        torch.save(self.state_dict(), path)

    @classmethod
    def load(cls, path, device="cuda", grad_hook=None):
        return cls.from_state_dict(torch.load(path, weights_only=True), device, grad_hook)
