"""Residual-TD3 learner on the GPU (robot.py:209-398), every FLOP in libnavenv.so kernels.

Method names follow the reference: td3_update, train_critic, train_actor, soft_update. Networks
live as DeviceMLP flat buffers; Adam moments live beside them; torch only allocates memory and
provides the stream. Sampling: robot.py:98-115 draws `batch_size` rows without replacement from a
<=10 000-row buffer; here rows are drawn with replacement by Philox (NAV_TAG_SAMPLE) from the
device ring, or taken from an injected index tensor (parity tests, the N=1 drop-in).
"""
import collections
import ctypes as C
import math

import torch

from . import config as K
from . import prof
from ._lib import NavReplay, descs, lib, parr, ptr, stream_handle
from .mlp import DeviceMLP

# the constant arguments of nav_td3_actor_rows, nav_td3_actor_rows_bc and nav_td3_actor_rows_bcq,
# by the ABI's names (q_demo / keep_part: the Q-filtered form's alone)
_ActorRows = collections.namedtuple(
    "_ActorRows", "actor critic batch q da bc_part acts save_mask dz dz_save_mask masks_actor "
                  "masks_critic edge_slabs q_demo keep_part", defaults=(None, None))


class _Adam:
    """torch.optim.Adam state for one flat parameter buffer (robot.py:236-239)."""

    def __init__(self, net, lr, betas=(0.9, 0.999), eps=1e-8):
        self.net, self.lr, self.b1, self.b2, self.eps = net, lr, betas[0], betas[1], eps
        self.m = torch.zeros_like(net.params)
        self.v = torch.zeros_like(net.params)
        self.step_count = 0

    def bias_corrections(self):
        """Count the next step t: its (1 - b1^t, sqrt(1 - b2^t))."""
        self.step_count += 1
        bc1 = 1 - self.b1 ** self.step_count
        bc2 = 1 - self.b2 ** self.step_count
        return bc1, math.sqrt(bc2)

    def advance(self):
        """Next step's (step_size, bc2_sqrt) = (lr / (1 - b1^t), sqrt(1 - b2^t))."""
        bc1, bc2_sqrt = self.bias_corrections()
        return self.lr / bc1, bc2_sqrt

    def step(self, grad, stream=None):
        ss, bc2s = self.advance()
        d = self.net.desc()
        lib().nav_adam(C.byref(d), ptr(grad), ptr(self.m), ptr(self.v), self.b1, self.b2,
                       self.eps, ss, bc2s, stream_handle(stream))

    def state_dict(self):
        return {"m": self.m.cpu(), "v": self.v.cpu(), "t": self.step_count}

    def load_state_dict(self, sd):
        self.m.copy_(sd["m"]); self.v.copy_(sd["v"]); self.step_count = sd["t"]


class TD3:
    def __init__(self, cfg=None, device="cuda", seed=K.RANDOM_SEED, actor=None, critic1=None,
                 critic2=None, grad_hook=None, wgrad_splits=None):
        self.cfg = cfg or K.TD3Config()
        c = self.cfg
        # every mode's refusals (TD3Config.check) and the hook's contract, before anything is
        # allocated; _static checks again once a mode field has changed
        c.check(grad_hook)
        self._checked = self._modes()
        # shared policy (BASELINE config 5): grad_hook(bucket) SUM-all-reduces a flat gradient
        # bucket in place (nav.dist.GradAllReduce: RCCL over xGMI) and Adam divides by the hook's
        # world_size. The contract is explicit: a hook without world_size is refused, since a
        # plain SUM callable would silently train on world_size x the mean gradient.
        self.grad_hook = grad_hook
        self.grad_div = 1.0
        if grad_hook is not None:
            ws = getattr(grad_hook, "world_size", None)
            if not isinstance(ws, int) or ws < 1:
                raise ValueError("grad_hook must carry an int world_size >= 1: it SUM-all-reduces "
                                 "the gradient bucket and Adam divides by world_size")
            self.grad_div = float(ws)
        nc = c.net
        self.device = torch.device(device)
        mk = lambda di, do: DeviceMLP(di, do, nc.hidden, nc.n_hidden, self.device)  # noqa: E731
        g = torch.Generator().manual_seed(seed)
        self.actor_network = actor or mk(2, 2).init_kaiming(g)
        self.critic_network_1 = critic1 or mk(4, 1).init_kaiming(g)
        self.critic_network_2 = critic2 or mk(4, 1).init_kaiming(g)
        # robot.py:232-234 deep copies
        self.target_actor = mk(2, 2).copy_from(self.actor_network)
        self.target_critic_network_1 = mk(4, 1).copy_from(self.critic_network_1)
        self.target_critic_network_2 = mk(4, 1).copy_from(self.critic_network_2)
        self.actor_optimizer = _Adam(self.actor_network, c.actor_lr)
        self.critic_optimizer_1 = _Adam(self.critic_network_1, c.critic_lr)
        self.critic_optimizer_2 = _Adam(self.critic_network_2, c.critic_lr)
        self.seed = seed
        self.update_counter = 0  # Philox counter for sampling / smoothing noise
        # learning from demonstrations (cfg.demo_fraction / bc_weight / q_weight; off by default)
        self.bc_counter = 0      # Philox counter of pretrain_bc's demonstration draws
        self.mix_launches = 0    # nav_td3_mix_idx launches issued (0 with the feature off)
        self._bc_ws = None       # bc_loss's workspace, by row count
        self._last_b_demo = 0    # demonstration rows of the last BC launch (bc_loss_value)
        # prioritised replay (cfg.per_alpha > 0) and multi-step returns (cfg.n_step > 1)
        self.per_launches = 0    # nav_per_* calls issued (0 with the feature off)
        self.nstep_launches = 0  # nav_nstep_rows calls issued (0 with the feature off)
        # row splits of the weight-gradient launches, (critic twins, actor); None = as many as
        # fill the chip (nav_mlp_wgrad_splits; tuning only)
        self.wgrad_splits = wgrad_splits
        # the twin online critics in separate workgroups: -1 = the library's choice by batch size
        # (1 / 0 force either form; the results are bit-identical)
        self.split_twins = -1
        self._B, self._ws_key = 0, None  # the workspace's batch size and key (_workspace)
        # every launch's constant ctypes arguments and work counts (_static), rebuilt when the
        # batch size, the seed or a hyper-parameter they carry changes (its key)
        self._st = None
        self._st_key = None
        self._rd = (None, None)
        # td3_update's collect_ready event while it is still to be recorded (_hook / the end)
        self._ready, self._ready_recorded = None, False
        self.actor_losses, self.critic_losses = [], []

    def _modes(self):
        return tuple(getattr(self.cfg, k) for k in K.MODE_FIELDS)

    # ---- workspace, keyed by all it allocates for: batch size, PER, n-step, the split counts
    def _workspace(self, B):
        d, hp, nh = self.device, self.actor_network.hp, self.actor_network.n_hidden
        L = lib()
        # row splits of the weight-gradient launch (partial slabs): critic twins and actor
        # separately, as many as fill the chip (wgrad_splits overrides; tuning only)
        sc = L.nav_mlp_wgrad_splits(2, self.critic_network_1.d_out, hp, nh, B)
        sa = L.nav_mlp_wgrad_splits(1, self.actor_network.d_out, hp, nh, B)
        if self.wgrad_splits:
            sc, sa = (max(1, min(int(v), max(1, B // 32))) for v in self.wgrad_splits)
        key = (B, self.per_on(), self.nstep_on(), sc, sa)
        if key == self._ws_key:
            return
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=d)  # noqa: E731
        self.batch = f(B, 8)
        self.batch2 = f(B, 8)
        self.q1 = f(B)
        self.dq1, self.dq2 = f(B), f(B)
        # saved rows: only hidden layers 1 .. nh-2; h_0 and the top dz are recomputed by the
        # weight-gradient kernel, the top layer's dWo partials come from registers
        self.acts1, self.acts2, self.acts_a = f(nh, B, hp), f(nh, B, hp), f(nh, B, hp)
        self.dz1, self.dz2, self.dz_a = f(nh, B, hp), f(nh, B, hp), f(nh, B, hp)
        self.mask1 = self.critic_network_1.mask_buffer(B)
        self.mask2 = self.critic_network_1.mask_buffer(B)
        self.mask_a = self.actor_network.mask_buffer(B)
        self.da = f(B, 2)
        self.nblk = L.nav_mlp_row_blocks(B)
        self.loss_part = f(2, self.nblk)
        # demonstrations: the epoch's mixed sample indices and the BC term's block sums
        self.idx_c = torch.zeros(B, dtype=torch.int64, device=d)
        self.idx_a = torch.zeros(B, dtype=torch.int64, device=d)
        self.bc_part = f(self.nblk)
        # the Q-filter: Q1(s, a) of the demonstration rows and the blocks' counts of kept rows
        self.q_demo = f(B)
        self.keep_part = torch.zeros(self.nblk, dtype=torch.int32, device=d)
        # prioritised replay: the batch's importance weights and the twins' |TD errors|
        if self.per_on():
            self.w_per, self.w_one = f(B), torch.ones(B, dtype=torch.float32, device=d)
            self.td_abs1, self.td_abs2 = f(B), f(B)
        # multi-step returns: the epoch's critic batch as n-step rows, their horizons, and the
        # indices 0 .. B-1 the critic launch reads them by
        if self.nstep_on():
            self.staged = f(B, 8)
            self.steps = torch.zeros(B, dtype=torch.int32, device=d)
            self.idx_iota = torch.arange(B, dtype=torch.int64, device=d)
            self._staged_rd = NavReplay(self.staged.data_ptr(), B)
        ec = L.nav_mlp_edge_count(4, 1, hp, nh)
        self.eslab1, self.eslab2 = f(self.nblk, ec), f(self.nblk, ec)
        self.eslab_a = f(self.nblk, L.nav_mlp_edge_count(2, 2, hp, nh))
        self.splits_c, self.splits_a = sc, sa
        hc = max(4, L.nav_mlp_hidden_count(hp, nh))
        self.hslab, self.hslab2 = f(max(sc, sa), hc), f(sc, hc)
        self.grad_a = f(self.actor_network.count)
        # the twin critics' flat gradients as ONE contiguous bucket (one all-reduce per epoch)
        cc = self.critic_network_1.count
        self.grad_c = f(2 * cc)
        self.grad_c1, self.grad_c2 = self.grad_c[:cc], self.grad_c[cc:]
        self._B, self._ws_key = B, key
        self._st = None

    # ---- the launches. Each is issued in one place, with its constant arguments and its work
    # count built once in _static (the small-batch learner of config 1 is bound by the host's
    # issue of ~450 launches per td3_update), through _run: timed or not, the same call
    def _run(self, name, work, fn, *args):
        """fn(*args), as the region `name` of an active timer (nav.prof) if there is one."""
        if prof._active is None:
            return fn(*args)
        with prof.region(name, work):
            return fn(*args)

    def _reduce_bytes(self, nets, eslabs, splits, adam):
        return sum(4.0 * (splits * (x.count - e.shape[1]) + e.numel() +
                          (4 if adam else 1) * x.count) for x, e in zip(nets, eslabs))

    def _group(self, nets, opts, inp, acts, dz, dy, ld_dy, masks, eslabs, grads, hslabs, splits,
               bucket, poly):
        """One net group's (the critic twins', the actor's) weight-gradient, reduce and Adam
        launches: (work, constant arguments) each."""
        n, net, B = len(nets), nets[0], self._B
        g = {"opts": opts, "floats": C.c_float * n, "bucket": bucket, "poly": poly, "wgrad": None}
        if net.n_hidden > 1:
            # k_wgrad_fact (d_out 1, 2 hidden layers, whole 64-wide tiles: 2 fp16 products per
            # f32 product) is timed apart from k_wgrad (3 products): their rooflines differ
            fact = net.d_out == 1 and net.n_hidden == 2 and net.hp % 64 == 0
            g["wgrad"] = ("mlp_wgrad_fact" if fact else "mlp_wgrad",
                          n * prof.mlp_wgrad_flops(net.hidden, net.n_hidden, B),
                          (descs(*nets), n, B, ptr(inp), 8, 0, parr(*acts), parr(*dz), parr(*dy),
                           ld_dy, parr(*masks), parr(*hslabs), splits))
        red = (descs(*nets), n, parr(*hslabs), splits, parr(*eslabs), self.nblk, parr(*grads))
        adam = (parr(*[o.m for o in opts]), parr(*[o.v for o in opts]), opts[0].b1, opts[0].b2,
                opts[0].eps)
        g["red"] = (self._reduce_bytes(nets, eslabs, splits, False), red)
        g["red_adam"] = (self._reduce_bytes(nets, eslabs, splits, True), red + adam)
        g["adam"] = (descs(*nets), n, parr(*grads)) + adam
        return g

    def _static(self):
        c = self.cfg
        B = c.batch_size
        key = (B, self.seed, c.policy_noise, c.noise_clip, c.max_action, c.gamma, c.tau,
               self.split_twins, c.bc_weight, c.q_weight, c.demo_fraction, c.per_alpha, c.n_step,
               c.bc_q_filter)
        if self._st is not None and self._st_key == key:
            return self._st
        if self._modes() != self._checked:  # a mode switched after construction
            c.check(self.grad_hook)
            self._checked = self._modes()
        self._workspace(B)
        c1, c2, a = self.critic_network_1, self.critic_network_2, self.actor_network
        t1, t2 = self.target_critic_network_1, self.target_critic_network_2
        ta, ca = self.target_actor.desc(), a.desc()
        c1d = c1.desc()
        mid, mida = c1.middle_layers(), a.middle_layers()
        h, nh = c1.hidden, c1.n_hidden
        fwd, bwd = prof.mlp_fwd_flops, prof.mlp_bwd_flops
        poly = (descs(self.target_actor), descs(t1, t2), descs(c1, c2), 2, c.tau)
        ar = _ActorRows(actor=C.byref(ca), critic=C.byref(c1d), batch=ptr(self.batch2),
                        q=ptr(self.q1), da=ptr(self.da), bc_part=ptr(self.bc_part),
                        acts=ptr(self.acts_a), save_mask=mida, dz=ptr(self.dz_a),
                        dz_save_mask=mida, masks_actor=ptr(self.mask_a),
                        masks_critic=ptr(self.mask1), edge_slabs=ptr(self.eslab_a),
                        q_demo=ptr(self.q_demo), keep_part=ptr(self.keep_part))
        st = {
            "keep": (ta, ca, c1d),
            "seed": (self.seed & 0xFFFFFFFF, (self.seed >> 32) & 0xFFFFFFFF),
            "cr_work": (fwd(2, 2, h, nh, B) + 4 * fwd(4, 1, h, nh, B) +
                        2 * bwd(4, 1, h, nh, B, False, True)),
            "cr_head": (C.byref(ta), descs(t1, t2), descs(c1, c2)),
            "cr_tail": (c.policy_noise, c.noise_clip, c.max_action, c.gamma, ptr(self.batch),
                        parr(self.dq1, self.dq2), parr(self.loss_part[0], self.loss_part[1]),
                        parr(self.eslab1, self.eslab2), parr(self.acts1, self.acts2), mid,
                        parr(self.mask1, self.mask2), 1, parr(self.dz1, self.dz2), mid,
                        self.split_twins),
            "ar_work": (fwd(2, 2, h, nh, B) + fwd(4, 1, h, nh, B) + bwd(4, 1, h, nh, B, True) +
                        bwd(2, 2, h, nh, B, False, True, True)),
            "ar": ar,  # and the critic-free BC form's (pretrain_bc)
            "ar_bc_alone": ar._replace(critic=None, q=None, masks_critic=None, q_demo=None,
                                       keep_part=None),
            "td_abs": parr(self.td_abs1, self.td_abs2) if self.per_on() else None,
            "c": self._group([c1, c2], (self.critic_optimizer_1, self.critic_optimizer_2),
                             self.batch, [self.acts1, self.acts2], [self.dz1, self.dz2],
                             [self.dq1, self.dq2], 1, [self.mask1, self.mask2],
                             [self.eslab1, self.eslab2], [self.grad_c1, self.grad_c2],
                             [self.hslab, self.hslab2], self.splits_c, self.grad_c, poly),
            "a": self._group([a], (self.actor_optimizer,), self.batch2, [self.acts_a],
                             [self.dz_a], [self.da], 2, [self.mask_a], [self.eslab_a],
                             [self.grad_a], [self.hslab], self.splits_a, self.grad_a, poly),
        }
        self._st, self._st_key = st, key
        return st

    def _replay_ref(self, replay):
        if self._rd[0] is not replay:
            d = replay.desc()
            self._rd = (replay, (d, C.byref(d)))
        return self._rd[1][1]

    def _wgrad(self, g, s):
        """Hidden x hidden weight gradients of the group's 1-2 same-shape nets: one MFMA launch
        writing `splits` partial slabs per net."""
        if g["wgrad"] is not None:
            name, work, args = g["wgrad"]
            self._run(name, work, lib().nav_mlp_wgrad, *args, s)

    def _reduce(self, g, s):
        """Fixed-order reduce of the weight-gradient slabs and the fwd/bwd edge partials into the
        group's flat gradients, no Adam."""
        work, args = g["red"]
        self._run("grad_reduce", work, lib().nav_grad_reduce_multi, *args, s)

    @staticmethod
    def _coeffs(g):
        """The group's next Adam steps: (step sizes, sqrt(1 - b2^t)) as float arrays."""
        ss, bc = zip(*[o.advance() for o in g["opts"]])
        return g["floats"](*ss), g["floats"](*bc)

    def _adam(self, g, s, grad_div=1.0, soft_update=False):
        """One multi-net Adam launch on flat gradients (already reduced) / grad_div; with
        soft_update the three soft updates in the same launch."""
        ss, bc = self._coeffs(g)
        if soft_update:
            lib().nav_adam_polyak_multi(*g["adam"], ss, bc, float(grad_div), *g["poly"], s)
        else:
            lib().nav_adam_multi(*g["adam"], ss, bc, float(grad_div), s)

    def _hook(self, bucket, stream):
        # the collective runs on torch's current stream: make it the launch stream, so it starts
        # after the reduce and Adam starts after it
        if self._ready is not None:  # the last epoch's replay reads and actor writes are issued
            self._ready.record(stream)
            self._ready, self._ready_recorded = None, True
        # region "allreduce": an event pair on the launch stream around the message (the
        # collective's stream waits for it and it for the collective), when a timer asks
        nbytes = bucket.numel() * bucket.element_size()
        if stream is None:
            self._run("allreduce", nbytes, self.grad_hook, bucket)
        else:
            with torch.cuda.stream(stream):
                self._run("allreduce", nbytes, self.grad_hook, bucket)

    def _step(self, g, s, stream, soft_update=False):
        """After a rows launch: the weight gradients, then the fixed-order reduce of those and
        the fwd/bwd edge partials fused with each net's Adam step (robot.py:236-239) of 1-2 nets
        (and on a policy epoch the three soft updates). With a grad_hook (shared policy) the
        reduce writes the flat gradient bucket without Adam, the hook all-reduces it, and one
        multi-net Adam launch applies bucket / world_size (and the soft updates)."""
        self._wgrad(g, s)
        if self.grad_hook is not None:
            self._reduce(g, s)
            self._hook(g["bucket"], stream)
            self._adam(g, s, self.grad_div, soft_update)
            return
        work, args = g["red_adam"]
        ss, bc = self._coeffs(g)
        if soft_update:  # the actor's step and all three soft updates in one launch
            self._run("grad_reduce", work, lib().nav_grad_reduce_adam_polyak, *args, ss, bc,
                      *g["poly"], s)
        else:
            self._run("grad_reduce", work, lib().nav_grad_reduce_adam, *args, ss, bc, s)

    # robot.py:312-366
    def _critic_rows(self, replay, idx, eps, s, w=None, staged=False):
        # sample + target actor with smoothing noise + twin target critics + TD target + online
        # twin forward with the MSE gradient + each online critic's row backward: one launch,
        # rows in LDS throughout. With w (prioritised replay) the weighted form: dq and the loss
        # carry w, the twins' |TD errors| go to td_abs1 / td_abs2. staged (multi-step returns):
        # the rows are self.staged's B rows in order, in place of `replay` and `idx`
        st = self._static()
        name, fn, tail = "critic_rows", lib().nav_td3_critic_rows, st["cr_tail"]
        if w is not None:
            name, fn = "critic_rows_w", lib().nav_td3_critic_rows_w
            tail += (ptr(w), st["td_abs"])
        if staged:
            ref, size, idx = C.byref(self._staged_rd), self._B, self.idx_iota
        else:
            ref, size = self._replay_ref(replay), len(replay)
        self._run(name, st["cr_work"], fn, *st["cr_head"], ref, size, self._B, ptr(idx),
                  *st["seed"], self.update_counter, ptr(eps), *tail, s)
        return st["c"]

    def _nstep_rows(self, replay, idx, s):
        """The epoch's critic batch as n-step rows into self.staged (nav_nstep_rows): row b from
        ring row idx[b], or from the index the critic launch would draw itself."""
        c = self.cfg
        self.nstep_launches += 1
        self._run("nstep_rows", 32.0 * (c.n_step + 2) * self._B, lib().nav_nstep_rows,
                  self._replay_ref(replay), ptr(replay.cut), len(replay), replay.position,
                  int(replay.stride), c.n_step, c.gamma, self._B, ptr(idx),
                  *self._static()["seed"], self.update_counter, ptr(self.staged),
                  ptr(self.steps), s)

    def train_critic(self, replay, idx=None, eps=None, stream=None):
        s = stream_handle(stream)
        # both critics' weight gradients, then reduce + Adam: one launch each
        self._step(self._critic_rows(replay, idx, eps, s), s, stream)

    def critic_gradients(self, replay, idx=None, eps=None, stream=None):
        """train_critic's gradient phase alone: both critics' flat gradients into the `grad_c`
        bucket ([critic 1 | critic 2], contiguous), no parameter changes. With critic_step this
        is train_critic's shared-policy path split where the collective goes."""
        s = stream_handle(stream)
        g = self._critic_rows(replay, idx, eps, s)
        self._wgrad(g, s)
        self._reduce(g, s)
        return self.grad_c

    def critic_step(self, grad_div=1.0, stream=None):
        """Adam on both critics from the `grad_c` bucket / grad_div (one launch)."""
        self._adam(self._static()["c"], stream_handle(stream), grad_div)

    def critic_loss_values(self):
        """(loss1, loss2) of the last train_critic (mean squared TD error), synchronising."""
        t = self.loss_part.sum(1) / self._B
        return t[0].item(), t[1].item()

    # robot.py:369-398
    @staticmethod
    def _actor_rows_call(a, sample, bc, q_filter=False):
        """(region, entry point, its arguments before the stream) from `a` (_ActorRows), `sample`
        = (replay, size, B, idx, seed_lo, seed_hi, counter) and `bc` = None (the plain form) or
        (B_demo, q_weight, bc_weight), with q_filter the Q-filtered BC form: each entry point's
        argument order, written once."""
        if q_filter:
            return "actor_rows_bcq", lib().nav_td3_actor_rows_bcq, (
                a.actor, a.critic, *sample, *bc, a.batch, a.q, a.da, a.bc_part, a.q_demo,
                a.keep_part, a.acts, a.save_mask, a.dz, a.dz_save_mask, a.masks_actor,
                a.masks_critic, a.edge_slabs)
        if bc is None:
            return "actor_rows", lib().nav_td3_actor_rows, (
                a.actor, a.critic, *sample, a.batch, a.q, a.da, a.acts, a.save_mask, a.dz,
                a.dz_save_mask, a.masks_actor, a.masks_critic, a.edge_slabs)
        return "actor_rows_bc", lib().nav_td3_actor_rows_bc, (
            a.actor, a.critic, *sample, *bc, a.batch, a.q, a.da, a.bc_part, a.acts, a.save_mask,
            a.dz, a.dz_save_mask, a.masks_actor, a.masks_critic, a.edge_slabs)

    def _actor_rows(self, replay, idx, s, bc=None, critic=True, ref=None, size=None):
        # sample + actor forward + critic-1 forward + backward of -mean(Q) to the action + the
        # actor's row backward with its edge partials: one launch. With bc = (B_demo, q_weight,
        # bc_weight) the BC form into the same workspace (critic False: the BC term alone; with
        # cfg.bc_q_filter and a critic its Q-filtered form);
        # ref / size: a replay descriptor and its fill in place of `replay`
        st = self._static()
        if bc is not None:
            self._last_b_demo = bc[0]
        if ref is None:
            ref, size = self._replay_ref(replay), len(replay)
        name, fn, args = self._actor_rows_call(
            st["ar"] if critic else st["ar_bc_alone"],
            (ref, size, self._B, ptr(idx), *st["seed"], self.update_counter), bc,
            bc is not None and critic and self.cfg.bc_q_filter)
        self._run(name, st["ar_work"], fn, *args, s)
        return st["a"]

    def _actor_rows_bc(self, critic, replay_ref, size, idx, b_demo, q_weight, bc_weight, s):
        """_actor_rows' BC form on a replay descriptor (critic False: the BC term alone)."""
        return self._actor_rows(None, idx, s, (b_demo, q_weight, bc_weight), critic, replay_ref,
                                size)

    def train_actor(self, replay, idx=None, stream=None, soft_update=False):
        """robot.py:369-398; with soft_update the three soft updates of robot.py:283-285 that
        follow it on a policy epoch ride in the actor's reduce + Adam launch."""
        s = stream_handle(stream)
        self._step(self._actor_rows(replay, idx, s), s, stream, soft_update)

    def actor_gradients(self, replay, idx=None, stream=None):
        """train_actor's gradient phase alone: the actor's flat gradient into `grad_a`."""
        s = stream_handle(stream)
        g = self._actor_rows(replay, idx, s)
        self._wgrad(g, s)
        self._reduce(g, s)
        return self.grad_a

    def actor_step(self, grad_div=1.0, stream=None):
        self._adam(self._static()["a"], stream_handle(stream), grad_div)

    def actor_loss_value(self):
        if not self.bc_on():
            return -(self.q1.sum() / self._B).item()
        return -self.cfg.q_weight * (self.q1.sum() / self._B).item() + \
            self.cfg.bc_weight * self.bc_loss_value()

    def bc_loss_value(self):
        """The last BC launch's term: sum_j (pi_j(s) - a_j)^2 averaged over its demonstration
        rows (0 without any), synchronising. With cfg.bc_q_filter the sum runs over the rows the
        filter kept; the divisor stays the demonstration rows."""
        n = self._last_b_demo
        return (self.bc_part.double().sum() / n).item() if n else 0.0

    def bc_kept_fraction(self):
        """The share of the last Q-filtered launch's demonstration rows whose BC term the filter
        kept, Q1(s, a) > Q1(s, pi(s)) (0.0 without demonstration rows or before any such
        launch), synchronising."""
        n = self._last_b_demo
        if not n or not self.cfg.bc_q_filter or not self._B:
            return 0.0
        return self.keep_part.sum().item() / n

    # ---- which modes are on (TD3Config's own)
    def per_on(self):
        return self.cfg.per_on()

    def nstep_on(self):
        return self.cfg.nstep_on()

    def bc_on(self):
        return self.cfg.bc_on()

    # ---- learning from demonstrations
    def b_demo(self):
        """Demonstration rows per batch: the batch's first round(demo_fraction * B) rows."""
        return self.cfg.b_demo()

    def _mix(self, size, b_demo, demo_base, n_demo, counter, idx_c, idx_a, s):
        self.mix_launches += 1
        self._run("mix_idx", 16.0 * self._B, lib().nav_td3_mix_idx, size, self._B, b_demo,
                  demo_base, n_demo, *self._static()["seed"], counter, ptr(idx_c), ptr(idx_a), s)

    def pretrain_bc(self, rows, epochs, batch=None, lr=None, stream=None):
        """Pure behaviour cloning of the actor on the demonstration rows `rows` [n][8] (the
        acting frame, DemoReplay.rows1): per epoch one nav_td3_mix_idx (every row of the batch a
        demonstration row), the critic-free BC form of the actor row kernel, then the actor's
        usual weight gradients, reduce and Adam step; at the end the target actor is the actor.
        batch: rows per epoch (default cfg.batch_size); lr: the actor's Adam step size for these
        epochs only. There is no critic here, so cfg.bc_q_filter does not apply: every row is
        cloned."""
        n = int(rows.shape[0])
        assert rows.shape == (n, 8) and rows.is_contiguous() and n >= 1
        c, opt = self.cfg, self.actor_optimizer
        keep = (c.batch_size, opt.lr)
        if batch is not None:
            c.batch_size = int(batch)
        if lr is not None:
            opt.lr = float(lr)
        s = stream_handle(stream)
        rd = NavReplay(rows.data_ptr(), n)
        try:
            self._static()
            B = self._B
            for _ in range(int(epochs)):
                self._mix(n, B, 0, n, self.bc_counter, None, self.idx_a, s)
                g = self._actor_rows_bc(False, C.byref(rd), n, self.idx_a, B, 0.0, 1.0, s)
                self._step(g, s, stream)
                self.bc_counter += 1
        finally:
            c.batch_size, opt.lr = keep
        self.target_actor.copy_from(self.actor_network)

    def bc_loss(self, rows, stream=None):
        """The BC term sum_j (pi_j(s) - a_j)^2 of the online actor averaged over all of `rows`
        [n][8], taken in order (idx = arange): deterministic. Changes no learner state. Unfiltered
        (no critic pass), whatever cfg.bc_q_filter says."""
        n = int(rows.shape[0])
        assert rows.shape == (n, 8) and rows.is_contiguous() and n >= 1
        a, L, d = self.actor_network, lib(), self.device
        if self._bc_ws is None or self._bc_ws["n"] != n:
            f = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=d)  # noqa: E731
            nblk = L.nav_mlp_row_blocks(n)
            mid = a.middle_layers()
            self._bc_ws = dict(
                n=n, idx=torch.arange(n, dtype=torch.int64, device=d), batch=f(n, 8), da=f(n, 2),
                acts=f(a.n_hidden, n, a.hp) if mid else None,
                dz=f(a.n_hidden, n, a.hp) if mid else None, mask=a.mask_buffer(n),
                part=f(nblk), es=f(nblk, L.nav_mlp_edge_count(2, 2, a.hp, a.n_hidden)), mid=mid)
        w = self._bc_ws
        rd = NavReplay(rows.data_ptr(), n)
        ad = a.desc()
        args = _ActorRows(actor=C.byref(ad), critic=None, batch=ptr(w["batch"]), q=None,
                          da=ptr(w["da"]), bc_part=ptr(w["part"]), acts=ptr(w["acts"]),
                          save_mask=w["mid"], dz=ptr(w["dz"]), dz_save_mask=w["mid"],
                          masks_actor=ptr(w["mask"]), masks_critic=None, edge_slabs=ptr(w["es"]))
        _, fn, args = self._actor_rows_call(args, (C.byref(rd), n, n, ptr(w["idx"]), 0, 0, 0),
                                            (n, 0.0, 1.0))
        fn(*args, stream_handle(stream))
        return (w["part"].double().sum() / n).item()

    # robot.py:293-310
    def soft_update(self, target, source, tau, stream=None):
        lib().nav_polyak(C.byref(target.desc()), C.byref(source.desc()), tau,
                         stream_handle(stream))

    def soft_update_all(self, stream=None):
        """The three soft updates of robot.py:283-285 in one launch."""
        t = self.cfg.tau
        lib().nav_polyak_multi(
            descs(self.target_actor, self.target_critic_network_1, self.target_critic_network_2),
            descs(self.actor_network, self.critic_network_1, self.critic_network_2), 3, t,
            stream_handle(stream))

    # robot.py:258-285
    def td3_update(self, replay, num_epochs=None, idx_fn=None, eps_fn=None, stream=None,
                   track_losses=False, collect_ready=None):
        """`collect_ready` (a torch.cuda.Event, optional) is recorded on `stream` at the first
        point after which nothing this update still has to issue reads the replay ring or writes
        the actor: with a grad_hook and a final epoch that is not a policy epoch, just before
        that epoch's critic all-reduce (so the next collect can run beside the collective and
        the critics' Adam step), otherwise at the end."""
        n = self.cfg.num_epochs if num_epochs is None else num_epochs
        self._ready, self._ready_recorded = None, False
        try:
            self._update(replay, n, idx_fn, eps_fn, stream, track_losses, collect_ready)
        finally:
            self._ready = None
            if collect_ready is not None and not self._ready_recorded:
                collect_ready.record(stream)

    def _update(self, replay, n, idx_fn, eps_fn, stream, track_losses, collect_ready):
        """The epoch loop of every mode; the modes differ in where the indices come from. Plain:
        the row launches draw their own. Demonstrations: one nav_td3_mix_idx (the first b_demo
        rows of both batches from the tail behind the ring), then the BC form of the actor
        launch. Prioritised replay: nav_per_sums, one nav_per_sample (both batches' indices, the
        critic batch's importance weights), the weighted critic launch, nav_per_update with the
        epoch's |TD errors|; the actor's loss stays unweighted. An explicit idx_fn wins: no mix
        (its first b_demo indices are taken to address demonstration rows), no sample (w = 1,
        the priorities still updated). Multi-step returns (n_step > 1) sit on top of the plain,
        prioritised and idx_fn modes: nav_nstep_rows stages the critic batch of those indices
        (None: the indices the launch would draw) as n-step rows, and the unchanged critic launch
        reads the staged rows in order, with its own counter and eps; the actor launch and
        nav_per_update keep the ring indices. Callbacks per epoch: idx_fn (critic batch), eps_fn, and
        once the critic phase is issued idx_fn (actor batch)."""
        if len(replay) < 1:
            return
        c, L = self.cfg, lib()
        bc, per, nstep = c.bc_on(), c.per_on(), c.nstep_on()
        if bc or per or nstep:  # the ring carries what the modes read (plain: its rows alone)
            replay.check_serves(c, injected=bool(idx_fn))
        if bc:
            b_demo, n_tail = c.b_demo(), int(replay.tail.shape[0])
        if per:
            pd = replay.per_ref()
        seed, B = self._static()["seed"], self._B
        s = stream_handle(stream)
        for epoch in range(n):
            policy = epoch % c.policy_update_delay == 0
            if (collect_ready is not None and epoch == n - 1 and self.grad_hook is not None and
                    not policy):
                self._ready = collect_ready
            # the epoch's indices (None: the row launches draw them) and the critic's weights
            idx_c = idx_a = w = None
            if per:
                self._run("per_sums", 4.0 * len(replay), L.nav_per_sums, pd, len(replay), s)
                self.per_launches += 1
            if idx_fn:
                idx_c, w = idx_fn(), (self.w_one if per else None)
            elif bc:
                idx_c, idx_a = self.idx_c, self.idx_a
                self._mix(len(replay), b_demo, replay.capacity, n_tail, self.update_counter,
                          idx_c, idx_a if policy else None, s)
            elif per:
                idx_c, idx_a, w = self.idx_c, (self.idx_a if policy else None), self.w_per
                self._run("per_sample", 16.0 * B, L.nav_per_sample, pd, len(replay), B, *seed,
                          self.update_counter, float(c.per_beta), ptr(idx_c), ptr(w), ptr(idx_a),
                          s)
                self.per_launches += 1
            if nstep:  # the critic batch staged as n-step rows; the launch reads them in order
                self._nstep_rows(replay, idx_c, s)
            g = self._critic_rows(replay, idx_c, eps_fn() if eps_fn else None, s, w, nstep)
            self._step(g, s, stream)
            if per:
                self._run("per_update", 20.0 * B, L.nav_per_update, pd, B, ptr(idx_c),
                          ptr(self.td_abs1), ptr(self.td_abs2), float(c.per_alpha),
                          float(c.per_eps), s)
                self.per_launches += 1
            if track_losses:
                self.critic_losses.append(sum(self.critic_loss_values()) / 2)
            if policy:
                if idx_fn:
                    idx_a = idx_fn()
                g = self._actor_rows(replay, idx_a, s,
                                     (b_demo, c.q_weight, c.bc_weight) if bc else None)
                # the three soft updates ride in the actor's reduce + Adam launch
                self._step(g, s, stream, soft_update=True)
                if track_losses:
                    self.actor_losses.append(self.actor_loss_value())
            self.update_counter += 1

    def networks(self):
        return {"actor": self.actor_network, "critic1": self.critic_network_1,
                "critic2": self.critic_network_2, "target_actor": self.target_actor,
                "target_critic1": self.target_critic_network_1,
                "target_critic2": self.target_critic_network_2}

    def state_dict(self):
        sd = {k: v.state_dict() for k, v in self.networks().items()}
        sd["opt"] = {k: o.state_dict() for k, o in (("actor", self.actor_optimizer),
                                                     ("critic1", self.critic_optimizer_1),
                                                     ("critic2", self.critic_optimizer_2))}
        sd["update_counter"] = self.update_counter
        if self.bc_counter:
            sd["bc_counter"] = self.bc_counter
        return sd

    def load_state_dict(self, sd):
        for k, v in self.networks().items():
            v.load_state_dict(sd[k])
        self.actor_optimizer.load_state_dict(sd["opt"]["actor"])
        self.critic_optimizer_1.load_state_dict(sd["opt"]["critic1"])
        self.critic_optimizer_2.load_state_dict(sd["opt"]["critic2"])
        self.update_counter = sd["update_counter"]
        self.bc_counter = sd.get("bc_counter", 0)
