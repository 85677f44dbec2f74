"""Vectorised Environment + Robot per-step state on one GPU (environment.py, robot.py:413-538).

`VecEnv` owns the structure-of-arrays per-env state as torch tensors (device memory) and drives the
gfx950 kernels of libnavenv.so through the C-ABI. One env = one lane; n envs advance per launch.
"""
import ctypes as C

import torch

from . import config as K
from . import prof
from ._lib import (NavEnvSoa, NavPer, NavReplay, NavStepOut, NavTestOut, lib, params_struct, ptr,
                   require_gpu, stream_handle)


def make_field(speed, angle, device="cuda"):
    """Interleave Environment.dynamics_speed / dynamics_angle ([100,100] float32, x-major) into the
    kernels' [100][100][2] table."""
    s = torch.as_tensor(speed, dtype=torch.float32)
    a = torch.as_tensor(angle, dtype=torch.float32)
    assert s.shape == (100, 100) and a.shape == (100, 100)
    return torch.stack([s, a], dim=-1).contiguous().to(device)


class DemoIndex:
    """Exact bucketed nearest-demo index (nav_demo_index_*): per (group, index cell) the list of
    demonstration points that can be nearest to any state in the cell. Two levels: the 1 x 1
    dynamics cells over every point of the group, then R x R index cells per dynamics cell
    (R = nav_demo_index_res()) over their parent's list. `cell_start` / `cand` are the index-cell
    lists the reward kernels walk. The indexed reward equals the brute-force one bit for bit
    (tests/test_gpu_env.py)."""

    L1_CELLS = 100 * 100

    def __init__(self, demo_xy, demo_off=None, stream=None):
        dev = demo_xy.device
        G = 1 if demo_off is None else demo_off.shape[0] - 1
        m = demo_xy.shape[0] if demo_off is None else 0
        s = stream_handle(stream)
        L = lib()
        self.res = int(L.nav_demo_index_res())
        self.side = 100 * self.res
        self.CELLS = self.side * self.side
        # level 1: dynamics cells over all points
        bound1 = torch.zeros(G * self.L1_CELLS, dtype=torch.float64, device=dev)
        count1 = torch.zeros(G * self.L1_CELLS, dtype=torch.int32, device=dev)
        start1 = torch.zeros(G * self.L1_CELLS + 1, dtype=torch.int64, device=dev)
        L.nav_demo_index_plan(ptr(demo_xy), ptr(demo_off), G, m, ptr(bound1), ptr(count1), s)
        L.nav_demo_index_scan(ptr(count1), G, ptr(start1), s)
        total1 = int(start1[-1].item())
        cand1 = torch.zeros(max(total1, 1), dtype=torch.int32, device=dev)
        L.nav_demo_index_fill(ptr(demo_xy), ptr(demo_off), G, m, ptr(bound1), ptr(start1),
                              ptr(cand1), s)
        # level 2: the query index
        bound = torch.zeros(G * self.CELLS, dtype=torch.float64, device=dev)
        count = torch.zeros(G * self.CELLS, dtype=torch.int32, device=dev)
        self.cell_start = torch.zeros(G * self.CELLS + 1, dtype=torch.int64, device=dev)
        L.nav_demo_index_subplan(ptr(demo_xy), ptr(demo_off), G, ptr(start1), ptr(cand1),
                                 ptr(bound), ptr(count), s)
        L.nav_demo_index_subscan(ptr(count), G, ptr(self.cell_start), s)
        total = int(self.cell_start[-1].item())
        self.cand = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
        L.nav_demo_index_subfill(ptr(demo_xy), ptr(demo_off), G, ptr(start1), ptr(cand1),
                                 ptr(bound), ptr(self.cell_start), ptr(self.cand), s)
        self.total = total
        self.total_l1 = total1
        self.mean_candidates = total / float(G * self.CELLS)

    def cell_of(self, g, x, y):
        """index cell of state (x, y) of group g (torch tensors), as the kernels compute it"""
        return g * self.CELLS + (x * self.res).long() * self.side + (y * self.res).long()


def ring_needs(cfg):
    """What a learner with cfg's modes reads beside the ring's rows, as ReplayRing's keywords
    (the tail's length is the caller's); ReplayRing.check_serves is the contract's other half."""
    return {"tail": cfg.bc_on(), "priorities": cfg.per_on(), "cuts": cfg.nstep_on()}


class ReplayRing:
    """ReplayBuffer (robot.py:58-124) as a device ring of 32-byte rows
    (s0 s1 a0 a1 r s'0 s'1 done, float32)."""

    def __init__(self, capacity, device="cuda", rows=None, tail=0, priorities=False, cuts=False):
        self.capacity = int(capacity)
        n_tail = int(tail)
        if rows is None:
            # `tail` demonstration rows behind the ring, in the same allocation: a sample index
            # k >= capacity addresses tail[k - capacity] through the row kernels' `idx`; desc(),
            # advance() and the ticks see the [capacity][8] ring alone
            self.storage = torch.zeros(self.capacity + n_tail, 8, dtype=torch.float32,
                                       device=device)
            rows = self.storage[:self.capacity]
        else:
            # (rows given: a [capacity + tail][8] slice of a population's ring tensor)
            assert rows.shape == (self.capacity + n_tail, 8) and rows.is_contiguous()
            self.storage = rows
            rows = self.storage[:self.capacity]
        assert rows.shape == (self.capacity, 8) and rows.is_contiguous()
        self.rows = rows
        self.tail = self.storage[self.capacity:]
        self.position = 0  # next write slot (robot.py:77)
        self.size = 0
        # prioritised replay: one u32 fixed-point priority per ring row (int32 storage), the sum
        # hierarchy's workspace and the four stat words (nav_per); none without `priorities`
        self.pri = self.sums = self.stat = None
        self._per = None
        if priorities:
            dev = self.rows.device
            self.pri = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
            self.sums = torch.zeros(lib().nav_per_sums_count(self.capacity), dtype=torch.int64,
                                    device=dev)
            self.stat = torch.zeros(4, dtype=torch.int32, device=dev)
            lib().nav_per_init(self.per_ref(), stream_handle())
        # multi-step returns: one u8 cut mark per ring row, 1 where the env was reset after that
        # row (nav_nstep_stamp), and the row distance between an env's consecutive transitions
        # (the trainer's n_envs; set by the trainer); none without `cuts`
        self.cut = None
        self.stride = None
        if cuts:
            self.cut = torch.zeros(self.capacity, dtype=torch.uint8, device=self.rows.device)

    def check_serves(self, cfg, injected=False):
        """ValueError unless this ring carries what cfg's modes read (ring_needs), once per
        update; `injected`: the caller gives the sample indices, demonstration rows among them."""
        if cfg.bc_on() and cfg.b_demo() and not injected and self.tail.shape[0] < 1:
            raise ValueError("demo_fraction > 0 needs a replay ring with a demonstration tail")
        if cfg.per_on() and self.pri is None:
            raise ValueError("per_alpha > 0 needs a replay ring with priorities "
                             "(ReplayRing(priorities=True))")
        if cfg.nstep_on():
            if self.cut is None:
                raise ValueError("n_step > 1 needs a replay ring with cut marks "
                                 "(ReplayRing(cuts=True))")
            if not self.stride:
                raise ValueError("n_step > 1 needs the ring's stride (ReplayRing.stride: the "
                                 "rows between an env's consecutive transitions, n_envs)")

    def desc(self):
        return NavReplay(self.rows.data_ptr(), self.capacity)

    def per_desc(self):
        return NavPer(self.pri.data_ptr(), self.sums.data_ptr(), self.stat.data_ptr(),
                      self.capacity)

    def per_ref(self):
        """byref of the (cached) nav_per descriptor"""
        if self._per is None:
            d = self.per_desc()
            self._per = (d, C.byref(d))
        return self._per[1]

    def stamp(self, base, n, stream=None, flags=None):
        """The rows a tick just pushed at `base` get the running maximum priority (on the
        tick's stream, by advance()'s caller); nothing without priorities. With cut marks and
        the tick's `flags` [n] u8, the rows' marks become the flags' bit 3 ('ended')."""
        if self.pri is not None:
            lib().nav_per_stamp(self.per_ref(), int(base), int(n), stream_handle(stream))
        if self.cut is not None and flags is not None:
            lib().nav_nstep_stamp(ptr(self.cut), self.capacity, int(base), int(n), ptr(flags),
                                  stream_handle(stream))

    def advance(self, n):
        base = self.position
        self.position = (self.position + n) % self.capacity
        self.size = min(self.size + n, self.capacity)
        return base

    def __len__(self):
        return self.size


class VecEnv:
    def __init__(self, n, field, seed=K.RANDOM_SEED, envs_per_group=1, demo_flag=True,
                 device="cuda", init=True, fuse_demo=True, **param_overrides):
        require_gpu()
        self.n = int(n)
        self.device = torch.device(device)
        self.field = field
        self.p = params_struct(seed_lo=seed & 0xFFFFFFFF, seed_hi=(seed >> 32) & 0xFFFFFFFF,
                               **param_overrides)
        self.envs_per_group = int(envs_per_group)
        d, n = self.device, self.n
        f64, i32 = torch.float64, torch.int32
        self.state = torch.zeros(n, 2, dtype=f64, device=d)
        self.goal = torch.zeros(n, 2, dtype=f64, device=d)
        self.region = torch.zeros(n, 4, dtype=f64, device=d)
        self.hist = torch.zeros(5, n, 2, dtype=f64, device=d)
        self.meta = torch.zeros(n, dtype=torch.int32, device=d)  # uint32 bits
        self.plan_index = torch.zeros(n, dtype=i32, device=d)
        self.path_length = torch.zeros(n, dtype=i32, device=d)
        self.episodes = torch.zeros(n, dtype=i32, device=d)
        self.noise_scale = torch.zeros(n, dtype=f64, device=d)
        # per-step outputs
        self.next_state = torch.zeros(n, 2, dtype=f64, device=d)
        self.goal_term = torch.zeros(n, dtype=f64, device=d)
        self.flags = torch.zeros(n, dtype=torch.uint8, device=d)
        self.block_stats = torch.zeros((n + 63) // 64, 8, dtype=torch.float32, device=d)
        self.goal_draws = torch.zeros(n, dtype=i32, device=d)
        self.soa = NavEnvSoa(n, *[t.data_ptr() for t in (
            self.state, self.goal, self.region, self.hist, self.meta, self.plan_index,
            self.path_length, self.episodes, self.noise_scale)])
        self.out = NavStepOut(self.next_state.data_ptr(), self.goal_term.data_ptr(),
                              self.flags.data_ptr(), self.block_stats.data_ptr())
        self.demo_xy = None
        self.demo_off = None
        self.demo_index = None
        self._shared_off = None  # a shared set's {0, m} offset table (set_demo)
        # demo reward fused into the tick launch (nav_agent_step_indexed); False keeps the two
        # launches (A/B and the fused-vs-unfused parity test)
        self.fuse_demo = bool(fuse_demo)
        self._test_out = {}  # (max_steps, traj) -> test_rollout's output tensors
        # resets to demonstration states (set_demo_resets): the stored set, the taken resets per
        # 64-env row (int64, cumulative; None until a set is stored) and the launches issued
        self._dreset = None
        self.demo_resets = None
        self.demo_reset_launches = 0
        if init:
            self.init(demo_flag)

    # environment.py:28-56 + robot.py:413-438 (vectorised, Philox)
    def init(self, demo_flag=True, stream=None):
        lib().nav_env_init(C.byref(self.p), C.byref(self.soa), self.envs_per_group,
                           int(bool(demo_flag)), ptr(self.goal_draws), stream_handle(stream))

    # environment.py:130-137
    def reset(self, mask=None, uniforms=None, stream=None):
        lib().nav_env_reset(C.byref(self.p), C.byref(self.soa), ptr(mask), ptr(uniforms),
                            stream_handle(stream))
        return self.state

    # environment.py:122-127 (pure Environment.step over all envs)
    def step(self, action, next_state=None, stream=None):
        with prof.region("env_step", float(prof.ENV_STEP_BYTES * self.n)):
            lib().nav_env_step(C.byref(self.p), C.byref(self.soa), ptr(self.field), ptr(action),
                               ptr(next_state), stream_handle(stream))
        return self.state

    # environment.py:122-127 applied K times in one launch (state in registers)
    def step_k(self, actions, next_states=None, stream=None):
        K = actions.shape[0]
        assert actions.shape == (K, self.n, 2) and actions.is_contiguous()
        with prof.region("env_step_k", float(prof.env_step_k_bytes(K, next_states is not None)
                                             * self.n)):
            lib().nav_env_step_k(C.byref(self.p), C.byref(self.soa), ptr(self.field),
                                 ptr(actions), K, ptr(next_states), stream_handle(stream))
        return self.state

    def dynamics(self, state, action, out=None, stream=None):
        out = out if out is not None else torch.empty_like(state)
        lib().nav_dynamics(ptr(self.field), ptr(state), ptr(action), ptr(out), state.shape[0],
                           stream_handle(stream))
        return out

    # demonstration set used by the demo-proximity reward (robot.py:749-757)
    def set_demo(self, demo_xy, demo_off=None, index=True):
        self.demo_xy = torch.as_tensor(demo_xy, dtype=torch.float64).reshape(-1, 2).contiguous()
        self.demo_xy = self.demo_xy.to(self.device)
        self.demo_off = None
        self._shared_off = None
        if demo_off is not None:
            self.demo_off = torch.as_tensor(demo_off, dtype=torch.int64).to(self.device)
        elif self.demo_xy.shape[0] > 0:
            # A shared set goes to the indexed entry points as one group of all envs: with
            # demo_off == NULL they carry no m, so a next state outside [0,100)^2 would find no
            # point to fall back to (navenv.h). The lists are the shared form's, entry for entry.
            self._shared_off = torch.tensor([0, self.demo_xy.shape[0]], dtype=torch.int64,
                                            device=self.device)
        self.demo_index = DemoIndex(self.demo_xy, self._index_groups()[0]) if index else None

    def _index_groups(self):
        """(demo_off, envs_per_group) as the indexed entry points take them"""
        if self.demo_off is None and self._shared_off is not None:
            return self._shared_off, max(self.n, 1)
        return self.demo_off, self.envs_per_group

    # resets to demonstration states (Nair et al. 2018): after every tick form, an env the tick
    # reset starts its new episode with probability `prob` on a state of one of its own group's
    # demonstrations (nav_demo_reset)
    def set_demo_resets(self, states, usable, prob, prob_group=None):
        """states [G * n_demos][T][2] float32, group-major (the CEM's demonstrations of the
        G = ceil(n / envs_per_group) env groups); usable [G * n_demos] int32, each in 1 .. T
        (nav.demos.demo_reset_usable); prob in [0, 1]; prob_group (optional, [G] values in
        [0, 1]) replaces prob per group. Stores the set on the device and allocates demo_resets;
        a later call replaces the set and keeps the counts. While every probability is 0 the
        ticks launch nothing."""
        G = (self.n + self.envs_per_group - 1) // self.envs_per_group
        st = torch.as_tensor(states, dtype=torch.float32).to(self.device).contiguous()
        us = torch.as_tensor(usable, dtype=torch.int32).to(self.device).contiguous()
        if st.dim() != 3 or st.shape[2] != 2 or st.shape[1] < 2 or st.shape[0] < G or \
                st.shape[0] % G != 0 or us.shape != (st.shape[0],):
            raise ValueError(f"demo resets need states [{G} * n_demos][T >= 2][2] and one usable "
                             f"count per demonstration; got {tuple(st.shape)}, {tuple(us.shape)}")
        T = int(st.shape[1])
        if int(us.min()) < 1 or int(us.max()) > T:
            raise ValueError(f"usable must lie in 1 .. T = {T}")
        prob = float(prob)
        if not 0.0 <= prob <= 1.0:
            raise ValueError(f"demo reset probability must lie in [0, 1], got {prob}")
        pg = None
        if prob_group is not None:
            pg = torch.as_tensor(prob_group, dtype=torch.float64).reshape(-1)
            if pg.shape[0] != G or not bool(((pg >= 0) & (pg <= 1)).all()):
                raise ValueError(f"prob_group must be {G} values in [0, 1]")
        on = prob > 0 if pg is None else bool((pg > 0).any())
        self._dreset = {"states": st, "usable": us, "n_demos": int(st.shape[0]) // G, "T": T,
                        "prob": prob, "prob_group": None if pg is None else pg.to(self.device),
                        "on": on}
        if self.demo_resets is None:
            self.demo_resets = torch.zeros((self.n + 63) // 64, dtype=torch.int64,
                                           device=self.device)

    def _demo_reset(self, stream=None):
        """nav_demo_reset on the tick's stream, iff a set is stored and some probability is > 0."""
        d = self._dreset
        if d is None or not d["on"]:
            return
        self.demo_reset_launches += 1
        lib().nav_demo_reset(C.byref(self.soa), ptr(self.flags), self.p.seed_lo, self.p.seed_hi,
                             ptr(d["states"]), ptr(d["usable"]), d["n_demos"], d["T"],
                             self.envs_per_group, d["prob"], ptr(d["prob_group"]),
                             ptr(self.demo_resets), stream_handle(stream))

    def demo_reset_share(self):
        """demo_resets.sum() / episodes.sum(): the episodes started on a demonstration state over
        the envs' episode numbers (which count from the reference's demonstration-phase episodes,
        nav_env_init). 0.0 without a stored set. Synchronises."""
        if self.demo_resets is None:
            return 0.0
        return float(self.demo_resets.sum().item()) / float(self.episodes.sum().item())

    # one fused training tick (robot.py:443-506, 645-675 + environment.py:122-137)
    def agent_step(self, action, replay, stream=None, reward_out=None):
        base = replay.position
        s = stream_handle(stream)
        rd = replay.desc()
        ix = self.demo_index if (self.demo_xy is not None and self.demo_xy.shape[0] > 0) else None
        if ix is not None and self.fuse_demo:
            # one launch: tick + indexed demo reward (bit-identical to the two-launch path)
            off, epg = self._index_groups()
            with prof.region("agent_step", float(prof.AGENT_STEP_BYTES * self.n)):
                lib().nav_agent_step_indexed(
                    C.byref(self.p), C.byref(self.soa), ptr(self.field), ptr(action), C.byref(rd),
                    base, C.byref(self.out), ptr(self.demo_xy), ptr(off), epg,
                    ptr(ix.cell_start), ptr(ix.cand), ptr(reward_out), s)
            replay.advance(self.n)
            replay.stamp(base, self.n, stream, self.flags)
            self._demo_reset(stream)
            return base
        has_demo = self.demo_xy is not None and self.demo_xy.shape[0] > 0
        with prof.region("agent_step", float(prof.AGENT_STEP_BYTES * self.n)):
            lib().nav_agent_step(C.byref(self.p), C.byref(self.soa), ptr(self.field),
                                 ptr(action), C.byref(rd), base, C.byref(self.out),
                                 int(has_demo), s)
        if has_demo:
            self.demo_reward(replay, base, reward_out=reward_out, stream=stream)
        replay.advance(self.n)
        replay.stamp(base, self.n, stream, self.flags)
        self._demo_reset(stream)
        return base

    # the two-launch tick's second launch: the demo-proximity term (robot.py:749-757) of the envs
    # the tick flagged, from next_state / goal_term / flags as they stand, into the rows at `base`
    def demo_reward(self, replay, base, reward_out=None, stream=None):
        s = stream_handle(stream)
        rd = replay.desc()
        ix = self.demo_index
        if ix is not None:
            off, epg = self._index_groups()
            # algorithmic work: the f64 ops over the candidates actually visited
            with prof.region("demo_reward", prof.demo_flops(self.n, ix.mean_candidates)):
                lib().nav_demo_reward_indexed(
                    C.byref(self.p), self.n, ptr(self.next_state), ptr(self.goal_term),
                    ptr(self.flags), ptr(self.demo_xy), ptr(off), epg, ptr(ix.cell_start),
                    ptr(ix.cand), C.byref(rd), base, ptr(reward_out), ptr(self.block_stats), s)
        else:
            m = self.demo_xy.shape[0] if self.demo_off is None else 0
            m_per = self.demo_xy.shape[0] if self.demo_off is None else \
                self.demo_xy.shape[0] / max(1, self.demo_off.shape[0] - 1)
            with prof.region("demo_reward", prof.demo_flops(self.n, m_per)):
                lib().nav_demo_reward(C.byref(self.p), self.n, ptr(self.next_state),
                                      ptr(self.goal_term), ptr(self.flags), ptr(self.demo_xy),
                                      ptr(self.demo_off), m, self.envs_per_group, C.byref(rd),
                                      base, ptr(reward_out), ptr(self.block_stats), s)

    # robot.py:541-569 + the training tick above, one launch (nav_act_tick): the actor's action
    # epilogue runs each env's tick in the same workgroup
    def act_tick(self, actor, step, replay, training=True, action_out=None, reward_out=None,
                 noise_z=None, stream=None):
        base = replay.position
        rd = replay.desc()
        a = actor.desc()
        ix = self.demo_index if (self.demo_xy is not None and self.demo_xy.shape[0] > 0) else None
        if self.demo_xy is not None and self.demo_xy.shape[0] > 0 and ix is None:
            raise ValueError("act_tick needs the demo index (set_demo(index=True))")
        flops = prof.mlp_fwd_flops(2, 2, actor.hidden, actor.n_hidden, self.n)
        off, epg = self._index_groups()
        with prof.region("act_tick", flops):
            lib().nav_act_tick(
                C.byref(self.p), C.byref(a), C.byref(self.soa), ptr(self.field), ptr(noise_z),
                int(step) & 0xFFFFFFFF, 0 if training else 1, C.byref(rd), base,
                C.byref(self.out), ptr(self.demo_xy) if ix else None,
                ptr(off) if ix else None, epg,
                ptr(ix.cell_start) if ix else None, ptr(ix.cand) if ix else None,
                ptr(action_out), ptr(reward_out), stream_handle(stream))
        replay.advance(self.n)
        replay.stamp(base, self.n, stream, self.flags)
        self._demo_reset(stream)
        return base

    # robot-learning.py:78, 104-117 for every env: one greedy test episode per env in ONE launch
    # (nav_test_rollout). Reads the goals (and the regions when the starts are drawn), never the
    # training state: the env SoA, the replay ring and the actor are left as they are.
    def test_rollout(self, actor, max_steps, episode=0, start=None, traj=False, stream=None):
        """Per-env device tensors of one test episode: reached [n] u8, steps [n] i32,
        best_distance [n] f64, final_state [n][2] f64 and (traj=True) traj [max_steps][n][2] f64.
        `start` [n][2] f64 gives the start states; None draws them from each env's init region on
        the test stream (NAV_TAG_TEST, `episode`). The tensors are allocated once per
        (max_steps, traj) and overwritten by the next call with the same pair."""
        max_steps = int(max_steps)
        out, o = self._test_tensors(max_steps, traj, start)
        a = actor.desc()
        flops = max_steps * prof.mlp_fwd_flops(2, 2, actor.hidden, actor.n_hidden, self.n)
        with prof.region("test_rollout", flops):
            lib().nav_test_rollout(C.byref(self.p), C.byref(a), C.byref(self.soa),
                                   ptr(self.field), ptr(start), int(episode) & 0xFFFFFFFF,
                                   max_steps, C.byref(o), stream_handle(stream))
        return out

    def _test_tensors(self, max_steps, traj, start):
        key = (max_steps, bool(traj))
        out = self._test_out.get(key)
        if out is None:
            d, n, f64 = self.device, self.n, torch.float64
            out = {"reached": torch.zeros(n, dtype=torch.uint8, device=d),
                   "steps": torch.zeros(n, dtype=torch.int32, device=d),
                   "best_distance": torch.zeros(n, dtype=f64, device=d),
                   "final_state": torch.zeros(n, 2, dtype=f64, device=d)}
            if traj:
                out["traj"] = torch.zeros(max_steps, n, 2, dtype=f64, device=d)
            self._test_out[key] = out
        if start is not None:
            assert start.shape == (self.n, 2) and start.dtype == torch.float64
        o = NavTestOut(*[ptr(out.get(k)) for k in ("reached", "steps", "best_distance",
                                                   "final_state", "traj")])
        return out, o

    # ---- populations (nav.population.PopulationTable): every member's launch form in one launch
    # act_tick with member m's actor, constants and ring on its envs (nav_act_tick_pop). `base`
    # is the rings' common write position; the caller advances the rings.
    def act_tick_pop(self, pop, step, base, training=True, action_out=None, reward_out=None,
                     noise_z=None, stream=None):
        assert pop.n_members * pop.envs_per_member == self.n and pop.replays is not None
        ix = self.demo_index if (self.demo_xy is not None and self.demo_xy.shape[0] > 0) else None
        if self.demo_xy is not None and self.demo_xy.shape[0] > 0 and ix is None:
            raise ValueError("act_tick_pop needs the demo index (set_demo(index=True))")
        net = pop.nets[0]
        flops = prof.mlp_fwd_flops(2, 2, net.hidden, net.n_hidden, self.n)
        with prof.region("act_tick_pop", flops):
            lib().nav_act_tick_pop(
                pop.params, pop.actors, pop.replays, pop.n_members, pop.envs_per_member,
                ptr(pop.table), C.byref(self.soa), ptr(self.field), ptr(noise_z),
                int(step) & 0xFFFFFFFF, 0 if training else 1, int(base), C.byref(self.out),
                ptr(self.demo_xy) if ix else None, ptr(self.demo_off) if ix else None,
                self.envs_per_group, ptr(ix.cell_start) if ix else None,
                ptr(ix.cand) if ix else None, ptr(action_out), ptr(reward_out),
                stream_handle(stream))
        self._demo_reset(stream)

    # test_rollout with member m's actor, max_action and goal_threshold on its envs
    # (nav_test_rollout_pop); the same output tensors as test_rollout
    def test_rollout_pop(self, pop, max_steps, episode=0, start=None, traj=False, stream=None):
        assert pop.n_members * pop.envs_per_member == self.n
        max_steps = int(max_steps)
        out, o = self._test_tensors(max_steps, traj, start)
        net = pop.nets[0]
        flops = max_steps * prof.mlp_fwd_flops(2, 2, net.hidden, net.n_hidden, self.n)
        with prof.region("test_rollout_pop", flops):
            lib().nav_test_rollout_pop(pop.params, pop.actors, pop.n_members,
                                       pop.envs_per_member, ptr(pop.table), C.byref(self.soa),
                                       ptr(self.field), ptr(start), int(episode) & 0xFFFFFFFF,
                                       max_steps, C.byref(o), stream_handle(stream))
        return out

    def stats(self):
        """Sum of the per-block rows: reward (the final pushed reward, demo term included, in
        every launch form: the demo-reward launches rewrite the reward column), done, goal,
        stuck, ended."""
        return self.block_stats.sum(0)[:5].tolist()
