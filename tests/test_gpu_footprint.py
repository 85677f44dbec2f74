"""Where the learner and acting launches store: every launch of the hot path under
tests/footprint.py's five checks (stray store, input preserved, written set, no dependence on prior
contents, same result as on zeroed exact-size tensors), at ragged row counts.

Each launch is described once by a builder: its entry point, one `Win` per pointer argument with
its role and the extent that include/navenv.h's own count functions give, and the expected
untouched set in closed form, each a sentence of the header:
 - acts / dz layers whose save_mask / dz_save_mask bit is clear;
 - columns of `out` outside [out_col, out_col + d_out) when ld_out > d_out;
 - edge-slab entries of the part a launch does not produce (nav_td3_critic_forward and
   nav_td3_critic_rows without its row backward write Wo | bo only; nav_mlp_backward without
   h_top writes everything but Wo | bo);
 - mask-image row tiles at or past nav_mlp_row_blocks(M) * (rows per block / 32);
 - q_demo rows >= B_demo; ring rows, cut and pri entries outside the written window.
Outputs passed as NULL have no window. Everything else must be written, by construction of check
3; params, m and v keep +0.0 on every padded slot after an optimizer step.

Shapes (hidden, n_hidden): (24, 1) padded width without hidden x hidden weights, (64, 2),
(200, 3) hp 224 with saved middle layers, (256, 2) the wide weight-gradient tile. Rows 1, 33, 100
(32-row workgroups) and, for (64, 2) and (256, 2), 16385 (64-row workgroups, the last one holding
one row and an empty second tile). Five weight-gradient splits of 32 rows leave split 4 of 100
rows and splits 2 .. 4 of 33 rows without a row. Inputs of a later stage (masks, saved rows,
slabs) come from the earlier launches run once on ordinary tensors and shared.

With NAV_FOOTPRINT_REPORT=<file> every case appends its id, wall time and findings there."""
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest

import footprint as F
import mlp_ref as R

pytestmark = pytest.mark.gpu
f32, f64, i64, i32, u32, u16, u8 = (np.float32, np.float64, np.int64, np.int32, np.uint32,
                                   np.uint16, np.uint8)
SEED = 1707366464
SLO, SHI = SEED & 0xFFFFFFFF, SEED >> 32
SHAPES = [(24, 1), (64, 2), (200, 3), (256, 2)]
BIG, BIG_SHAPES = 16385, [(64, 2), (256, 2)]
RING = 500
KINDS = {"actor": (2, 2), "critic": (4, 1)}
CASES = []


def case(cid, fn, **kw):
    CASES.append(pytest.param(fn, kw, id=cid))


def rows_of(shape):
    return [1, 33, 100] + ([BIG] if shape in BIG_SHAPES else [])


def lib():
    from nav._lib import lib as _l
    return _l()


def stream():
    from nav._lib import stream_handle
    return stream_handle()


def pad32(h):
    return (h + 31) // 32 * 32


def parr(*ptrs):
    return (C.c_void_p * len(ptrs))(*[None if p is None else p.addr for p in ptrs])


def farr(*v):
    return (C.c_float * len(v))(*v)


# ---------------------------------------------------------------- networks and shared data
def device_image(layers, d_in, d_out, hidden, nh):
    """(params, packed) of the network as the library lays them out, on the host."""
    import torch
    from nav.mlp import DeviceMLP
    net = DeviceMLP(d_in, d_out, hidden, nh, "cuda").load(layers)
    torch.cuda.synchronize()
    npk = lib().nav_mlp_packed_count(net.hp, nh)
    return net.params.cpu().numpy(), (net.packed.cpu().numpy()[:npk] if npk else None)


class Net:
    def __init__(self, seed, d_in, d_out, hidden, nh):
        from oracle.td3_oracle import make_mlp_params
        self.d_in, self.d_out, self.hidden, self.nh = d_in, d_out, hidden, nh
        self.hp = pad32(hidden)
        layers = make_mlp_params(seed, [d_in] + [hidden] * nh + [d_out])
        self.params, self.packed = device_image(layers, d_in, d_out, hidden, nh)
        self.offs, self.count = R.layer_offsets(d_in, d_out, self.hp, nh)
        assert self.count == self.params.size == lib().nav_mlp_param_count(d_in, d_out, self.hp, nh)
        self.hw = (nh - 1) * self.hp * self.hp
        assert self.hw == lib().nav_mlp_hidden_count(self.hp, nh)
        self.ec = self.count - self.hw
        assert self.ec == lib().nav_mlp_edge_count(d_in, d_out, self.hp, nh)
        self.e_wo = self.offs[nh][0] - self.hw
        self.logical = R.logical_mask(d_in, d_out, hidden, self.hp, nh).numpy()

    def wins(self, name, role="in", role_k=None):
        w = {name + ".p": F.Win(self.count, f32, role, init=self.params)}
        if self.packed is not None:
            rk = role_k or role
            w[name + ".k"] = F.Win(self.packed.size, f32, rk, pitch=self.hp,
                                   init=None if rk == "out" else self.packed)
        return w

    def desc(self, b, name):
        from nav._lib import NavMlp
        k = b[name + ".k"].addr if self.packed is not None else None
        return NavMlp(self.d_in, self.d_out, self.hidden, self.hp, self.nh, b[name + ".p"].addr, k)

    def split_flat(self, flat):
        """A flat [.., count] array as its (edge, hidden) slab parts."""
        hid = np.zeros(self.count, bool)
        for l in range(1, self.nh):
            hid[self.offs[l][0]:self.offs[l][0] + self.hp * self.hp] = True
        return flat[..., ~hid], flat[..., hid]


def descs(b, *named):
    from nav._lib import NavMlp
    return (NavMlp * len(named))(*[n.desc(b, name) for n, name in named])


@functools.lru_cache(maxsize=None)
def nets(hidden, nh):
    return {name: Net(seed, *(KINDS["actor"] if name in ("ta", "actor", "atgt") else
                              KINDS["critic"]), hidden, nh)
            for name, seed in R.EPOCH_SEEDS.items()}


@functools.lru_cache(maxsize=None)
def data(B, variant=0):
    """A ring of RING rows (done ~ 10 %), injected sample indices of both phases and smoothing
    noise."""
    g = np.random.default_rng(9000 + B + 7919 * variant)
    rows = (g.standard_normal((RING, 8)) * 10).astype(f32)
    rows[:, 7] = g.random(RING) < 0.1
    return dict(rows=rows, idx=g.integers(0, RING, B), idx_a=g.integers(0, RING, B),
                eps=g.standard_normal((B, 2)).astype(f32))


def run_plain(wins, launch):
    """The launch on ordinary zeroed tensors: name -> host array (a later stage's inputs)."""
    mem = F.TorchMem()
    b = F.bind(wins, mem, "plain")
    launch(b)
    mem.sync()
    return {k: np.ascontiguousarray(v.snapshot()[1]).view(wins[k].dtype) for k, v in b.items()}


def device_table(nbytes):
    """Zeroed device memory for a population table: (keep-alive object, address)."""
    import torch
    t = torch.zeros(int(nbytes), dtype=torch.uint8, device="cuda")
    return t, C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------- expected untouched sets
def rt_of(M):
    return 1 if M <= 16384 else 2


def mask_untouched(hp, nh, M):
    """Row tiles at or past (rows per workgroup / 32) * nav_mlp_row_blocks(M): every workgroup
    writes the words of all its row tiles, the empty second tile of a last 64-row block too."""
    n_rt = (M + 127) // 128 * 4
    m = np.ones((nh, n_rt, hp // 32 * 64), bool)
    m[:, :rt_of(M) * lib().nav_mlp_row_blocks(M)] = False
    assert m.size == lib().nav_mlp_mask_count(hp, nh, M)
    return m.reshape(-1)


def layers_untouched(nh, M, hp, save_mask):
    m = np.ones((nh, M * hp), bool)
    for l in range(nh):
        if (save_mask >> l) & 1:
            m[l] = False
    return m.reshape(-1)


def edge_untouched(net, nblk, part):
    """part 'top': only Wo | bo written; 'low': everything but Wo | bo written; 'all'."""
    m = np.zeros((nblk, net.ec), bool)
    if part == "top":
        m[:, :net.e_wo] = True
    elif part == "low":
        m[:, net.e_wo:] = True
    return m.reshape(-1)


def mid_of(nh):
    return sum(1 << l for l in range(1, nh - 1))


def rows_wins(net, M, tag, role="out", init=None):
    """acts / dz style [n_hidden][M][hp] window."""
    return F.Win(net.nh * M * net.hp, f32, role, pitch=net.hp, init=init)


def mask_win(net, M, role="out", init=None):
    return F.Win(lib().nav_mlp_mask_count(net.hp, net.nh, M), np.uint16, role,
                 pitch=net.hp // 32 * 64, init=init)


# ---------------------------------------------------------------- the unfused chain
def b_forward(hidden, nh, M, kind, n_nets, out_mode, ld_out, out_col, save_mask):
    ns = nets(hidden, nh)
    named = [(ns["actor"], "n0")] if kind == "actor" else [(ns["cr0"], "n0"), (ns["cr1"], "n1")]
    named = named[:n_nets]
    net = named[0][0]
    d = data(M)
    wins = {"in": F.Win(M * 8, f32, "in", pitch=8, init=d["rows"][d["idx"]]),
            "eps": F.Win(M * 2, f32, "in", pitch=2, init=d["eps"])}
    unt = {}
    for i, (n, name) in enumerate(named):
        wins.update(n.wins(name))
        wins[f"out{i}"] = F.Win(M * ld_out, f32, "out", pitch=ld_out)
        wins[f"acts{i}"] = rows_wins(n, M, "acts")
        wins[f"masks{i}"] = mask_win(n, M)
        o = np.ones((M, ld_out), bool)
        o[:, out_col:out_col + n.d_out] = False
        unt[f"out{i}"] = o
        unt[f"acts{i}"] = layers_untouched(nh, M, n.hp, save_mask)
        unt[f"masks{i}"] = mask_untouched(n.hp, nh, M)
    k = len(named)

    def launch(b):
        lib().nav_mlp_forward(descs(b, *named), k, M, b["in"].ptr, 8, 0,
                              parr(*[b[f"out{i}"] for i in range(k)]), ld_out, out_col, out_mode,
                              b["eps"].ptr, 0.2, 0.5, 5.0, SLO, SHI, 3,
                              parr(*[b[f"acts{i}"] for i in range(k)]), save_mask,
                              parr(*[b[f"masks{i}"] for i in range(k)]), stream())
    return wins, launch, unt, None


@functools.lru_cache(maxsize=None)
def fwd_state(hidden, nh, M, kind):
    """The forward's masks and saved rows (every layer) for the backward cases."""
    wins, launch, _, _ = b_forward(hidden, nh, M, kind, 2 if kind == "critic" else 1, 0,
                                   KINDS[kind][1], 0, (1 << nh) - 1)
    return run_plain(wins, launch)


def b_critic_forward(hidden, nh, B):
    ns = nets(hidden, nh)
    named = [(ns["cr0"], "n0"), (ns["cr1"], "n1")]
    net = ns["cr0"]
    d = data(B)
    nblk = lib().nav_mlp_row_blocks(B)
    g = np.random.default_rng(B)
    batch = d["rows"][d["idx"]]
    wins = {"in": F.Win(B * 8, f32, "in", pitch=8, init=batch),
            "q1t": F.Win(B, f32, "in", init=g.standard_normal(B)),
            "q2t": F.Win(B, f32, "in", init=g.standard_normal(B))}
    unt = {}
    for i, (n, name) in enumerate(named):
        wins.update(n.wins(name))
        wins[f"dq{i}"] = F.Win(B, f32, "out")
        wins[f"lp{i}"] = F.Win(nblk, f32, "out")
        wins[f"es{i}"] = F.Win(nblk * n.ec, f32, "out", pitch=n.ec)
        wins[f"acts{i}"] = rows_wins(n, B, "acts")
        wins[f"masks{i}"] = mask_win(n, B)
        unt[f"es{i}"] = edge_untouched(n, nblk, "top")
        unt[f"masks{i}"] = mask_untouched(n.hp, nh, B)
    two = lambda b, k: parr(b[k + "0"], b[k + "1"])  # noqa: E731

    def launch(b):
        lib().nav_td3_critic_forward(descs(b, *named), B, b["in"].ptr, 8, 0, b["in"].ptr,
                                     b["q1t"].ptr, b["q2t"].ptr, 0.99, two(b, "dq"), two(b, "lp"),
                                     two(b, "es"), two(b, "acts"), (1 << nh) - 1, two(b, "masks"),
                                     stream())
    return wins, launch, unt, None


def b_backward(hidden, nh, M, kind, dx, h_top, save_mask):
    ns = nets(hidden, nh)
    named = [(ns["actor"], "n0")] if kind == "actor" else [(ns["cr0"], "n0"), (ns["cr1"], "n1")]
    k = len(named)
    st = fwd_state(hidden, nh, M, kind)
    d = data(M)
    nblk = lib().nav_mlp_row_blocks(M)
    g = np.random.default_rng(M + 1)
    wins = {"in": F.Win(M * 8, f32, "in", pitch=8, init=d["rows"][d["idx"]])}
    unt = {}
    for i, (n, name) in enumerate(named):
        wins.update(n.wins(name))
        wins[f"dy{i}"] = F.Win(M * n.d_out, f32, "in", pitch=n.d_out,
                               init=g.standard_normal(M * n.d_out) / M)
        wins[f"masks{i}"] = mask_win(n, M, "in", st[f"masks{i}"])
        if h_top:
            top = st[f"acts{i}"].reshape(nh, M * n.hp)[nh - 1]
            wins[f"htop{i}"] = F.Win(M * n.hp, f32, "in", pitch=n.hp, init=top)
        wins[f"dz{i}"] = rows_wins(n, M, "dz")
        unt[f"dz{i}"] = layers_untouched(nh, M, n.hp, save_mask)
        if dx:
            wins[f"dx{i}"] = F.Win(M * n.d_in, f32, "out", pitch=n.d_in)
        wins[f"es{i}"] = F.Win(nblk * n.ec, f32, "out", pitch=n.ec)
        unt[f"es{i}"] = edge_untouched(n, nblk, "all" if h_top else "low")
    ld_dy = named[0][0].d_out

    def launch(b):
        each = lambda key: parr(*[b[f"{key}{i}"] for i in range(k)])  # noqa: E731
        lib().nav_mlp_backward(descs(b, *named), k, M, each("dy"), ld_dy, each("masks"),
                               b["in"].ptr, 8, 0, each("htop") if h_top else None, each("dz"),
                               save_mask, each("dx") if dx else None, each("es"), stream())
    return wins, launch, unt, None


# ---------------------------------------------------------------- the fused rows
def b_critic_rows(hidden, nh, B, row_backward, split_twins, weighted=False, variant=0):
    ns = nets(hidden, nh)
    cr = [(ns["cr0"], "cr0"), (ns["cr1"], "cr1")]
    tc = [(ns["tc0"], "tc0"), (ns["tc1"], "tc1")]
    net = ns["cr0"]
    d = data(B, variant)
    mid = mid_of(nh)
    nblk = lib().nav_mlp_row_blocks(B)
    wins = {"ring": F.Win(RING * 8, f32, "in", pitch=8, init=d["rows"]),
            "idx": F.Win(B, i64, "in", init=d["idx"]),
            "eps": F.Win(B * 2, f32, "in", pitch=2, init=d["eps"]),
            "batch": F.Win(B * 8, f32, "out", pitch=8)}
    wins.update(ns["ta"].wins("ta"))
    unt = {}
    for i in range(2):
        wins.update(cr[i][0].wins(cr[i][1]))
        wins.update(tc[i][0].wins(tc[i][1]))
        wins[f"dq{i}"] = F.Win(B, f32, "out")
        wins[f"lp{i}"] = F.Win(nblk, f32, "out")
        wins[f"es{i}"] = F.Win(nblk * net.ec, f32, "out", pitch=net.ec)
        wins[f"acts{i}"] = rows_wins(net, B, "acts")
        wins[f"dz{i}"] = rows_wins(net, B, "dz")
        wins[f"masks{i}"] = mask_win(net, B)
        unt[f"es{i}"] = edge_untouched(net, nblk, "all" if row_backward else "top")
        unt[f"acts{i}"] = layers_untouched(nh, B, net.hp, mid)
        unt[f"dz{i}"] = layers_untouched(nh, B, net.hp, mid if row_backward else 0)
        unt[f"masks{i}"] = mask_untouched(net.hp, nh, B)
        if weighted:
            wins[f"td{i}"] = F.Win(B, f32, "out")
    if weighted:
        wins["w"] = F.Win(B, f32, "in",
                          init=np.random.default_rng(B).uniform(0.25, 1.0, B))
    two = lambda b, k: parr(b[k + "0"], b[k + "1"])  # noqa: E731

    def launch(b):
        from nav._lib import NavReplay
        rd = NavReplay(b["ring"].addr, RING)
        args = [C.byref(ns["ta"].desc(b, "ta")), descs(b, *tc), descs(b, *cr), C.byref(rd), RING,
                B, b["idx"].ptr, SLO, SHI, 3, b["eps"].ptr, 0.2, 0.5, 5.0, 0.99, b["batch"].ptr,
                two(b, "dq"), two(b, "lp"), two(b, "es"), two(b, "acts"), mid, two(b, "masks"),
                row_backward, two(b, "dz"), mid, split_twins]
        if weighted:
            lib().nav_td3_critic_rows_w(*args, b["w"].ptr, two(b, "td"), stream())
        else:
            lib().nav_td3_critic_rows(*args, stream())
    return wins, launch, unt, None


def b_actor_rows(hidden, nh, B, form="plain", B_demo=0, critic=True, q_demo=True, variant=0):
    ns = nets(hidden, nh)
    actor, cr = ns["actor"], ns["cr0"]
    d = data(B, variant)
    mid = mid_of(nh)
    nblk = lib().nav_mlp_row_blocks(B)
    wins = {"ring": F.Win(RING * 8, f32, "in", pitch=8, init=d["rows"]),
            "idx": F.Win(B, i64, "in", init=d["idx_a"]),
            "batch": F.Win(B * 8, f32, "out", pitch=8),
            "da": F.Win(B * 2, f32, "out", pitch=2),
            "acts": rows_wins(actor, B, "acts"), "dz": rows_wins(actor, B, "dz"),
            "ma": mask_win(actor, B), "es": F.Win(nblk * actor.ec, f32, "out", pitch=actor.ec)}
    wins.update(actor.wins("actor"))
    unt = {"acts": layers_untouched(nh, B, actor.hp, mid),
           "dz": layers_untouched(nh, B, actor.hp, mid),
           "ma": mask_untouched(actor.hp, nh, B)}
    if critic:
        wins.update(cr.wins("cr0"))
        wins["q"] = F.Win(B, f32, "out")
        wins["mc"] = mask_win(cr, B)
        unt["mc"] = mask_untouched(cr.hp, nh, B)
    if form != "plain":
        wins["bc_part"] = F.Win(nblk, f32, "out")
    if form == "bcq":
        wins["keep_part"] = F.Win(nblk, i32, "out")
        if q_demo:
            wins["q_demo"] = F.Win(B, f32, "out")
            unt["q_demo"] = np.arange(B) >= B_demo
    bc_w = 0.5 if B_demo else 0.0
    opt = lambda b, k: b[k].ptr if k in b else None  # noqa: E731

    def launch(b):
        from nav._lib import NavReplay
        rd = NavReplay(b["ring"].addr, RING)
        head = [C.byref(actor.desc(b, "actor")), C.byref(cr.desc(b, "cr0")) if critic else None,
                C.byref(rd), RING, B, b["idx"].ptr, SLO, SHI, 3]
        tail = [b["acts"].ptr, mid, b["dz"].ptr, mid, b["ma"].ptr, opt(b, "mc"), b["es"].ptr,
                stream()]
        if form == "plain":
            lib().nav_td3_actor_rows(*head, b["batch"].ptr, b["q"].ptr, b["da"].ptr, *tail)
        elif form == "bc":
            lib().nav_td3_actor_rows_bc(*head, B_demo, 1.0, bc_w, b["batch"].ptr, opt(b, "q"),
                                        b["da"].ptr, b["bc_part"].ptr, *tail)
        else:
            lib().nav_td3_actor_rows_bcq(*head, B_demo, 1.0, bc_w, b["batch"].ptr, b["q"].ptr,
                                         b["da"].ptr, b["bc_part"].ptr, opt(b, "q_demo"),
                                         b["keep_part"].ptr, *tail)
    return wins, launch, unt, None


@functools.lru_cache(maxsize=None)
def critic_state(hidden, nh, B, variant=0):
    wins, launch, _, _ = b_critic_rows(hidden, nh, B, 1, -1, variant=variant)
    return run_plain(wins, launch)


@functools.lru_cache(maxsize=None)
def actor_state(hidden, nh, B, variant=0):
    wins, launch, _, _ = b_actor_rows(hidden, nh, B, variant=variant)
    return run_plain(wins, launch)


def b_wgrad(hidden, nh, B, group, splits):
    """group 'critic': the twin critics from the critic rows' state; 'actor': from the actor's.
    splits 0: nav_mlp_wgrad_splits."""
    ns = nets(hidden, nh)
    if group == "critic":
        named, st = [(ns["cr0"], "cr0"), (ns["cr1"], "cr1")], critic_state(hidden, nh, B)
        key = lambda k, i: f"{k}{i}"  # noqa: E731
        dyk, mk = "dq", "masks"
    else:
        named, st = [(ns["actor"], "actor")], actor_state(hidden, nh, B)
        key = lambda k, i: k  # noqa: E731
        dyk, mk = "da", "ma"
    net = named[0][0]
    k = len(named)
    if not splits:
        splits = int(lib().nav_mlp_wgrad_splits(k, net.d_out, net.hp, nh, B))
    wins = {"in": F.Win(B * 8, f32, "in", pitch=8, init=st["batch"])}
    for i, (n, name) in enumerate(named):
        wins.update(n.wins(name))
        wins[f"acts{i}"] = rows_wins(n, B, "acts", "in", st[key("acts", i)])
        wins[f"dz{i}"] = rows_wins(n, B, "dz", "in", st[key("dz", i)])
        wins[f"dy{i}"] = F.Win(B * n.d_out, f32, "in", pitch=n.d_out, init=st[key(dyk, i)])
        wins[f"masks{i}"] = mask_win(n, B, "in", st[key(mk, i)])
        wins[f"hs{i}"] = F.Win(splits * n.hw, f32, "out", pitch=n.hp)

    def launch(b):
        each = lambda kk: parr(*[b[f"{kk}{i}"] for i in range(k)])  # noqa: E731
        lib().nav_mlp_wgrad(descs(b, *named), k, B, b["in"].ptr, 8, 0, each("acts"), each("dz"),
                            each("dy"), net.d_out, each("masks"), each("hs"), splits, stream())

    def post(vals):
        """A split whose rows [s * P, (s + 1) * P), P = ceil(B / splits) rounded up to 32, lie at
        or past B holds zeros (the factored kernel's Wo[n] / 2 * 0 is -0.0 where Wo[n] < 0)."""
        per = (-(-B // splits) + 31) // 32 * 32
        out = []
        for i in range(k):
            hs = vals[f"hs{i}"].reshape(splits, -1)
            for sp in range(splits):
                if sp * per >= B and (hs[sp] != 0).any():
                    out.append(("non-zero empty split", f"hs{i} split {sp}"))
        return out
    return wins, launch, {}, post


# ---------------------------------------------------------------- the optimizer side
def slabs_for(net, blocks, splits, seed):
    """Random edge slabs [blocks][ec] and hidden slabs [splits][hw] with exact zeros on every
    padded slot, as the row and weight-gradient kernels produce them."""
    g = np.random.default_rng(seed)
    e, _ = net.split_flat((g.standard_normal((blocks, net.count)) * net.logical).astype(f32))
    _, h = net.split_flat((g.standard_normal((splits, net.count)) * net.logical).astype(f32))
    return e, (h if net.hw else np.zeros(4, f32))


def moments(net, seed):
    g = np.random.default_rng(seed)
    return ((g.standard_normal(net.count) * 1e-3 * net.logical).astype(f32),
            (g.random(net.count) * 1e-4 * net.logical).astype(f32))


def pads_zero(names_nets):
    """post check: every padded slot of the named windows holds +0.0 (all bits clear)."""
    def post(vals):
        out = []
        for name, net in names_nets:
            bad = (vals[name].view(np.uint32) != 0) & ~net.logical
            if bad.any():
                out.append(("non-zero pad slot", f"{name}: {int(bad.sum())} slot(s), first at "
                                                 f"{np.flatnonzero(bad)[:6].tolist()}"))
        return out
    return post


def b_reduce(hidden, nh, blocks, form, splits=3):
    """form 'one': nav_grad_reduce (the actor); 'multi': nav_grad_reduce_multi (twin critics)."""
    ns = nets(hidden, nh)
    named = [(ns["actor"], "n0")] if form == "one" else [(ns["cr0"], "n0"), (ns["cr1"], "n1")]
    k = len(named)
    wins = {}
    for i, (n, name) in enumerate(named):
        e, h = slabs_for(n, blocks, splits, 100 * blocks + i)
        wins.update(n.wins(name))
        wins[f"es{i}"] = F.Win(e.size, f32, "in", pitch=n.ec, init=e)
        wins[f"hs{i}"] = F.Win(h.size, f32, "in", pitch=n.hp, init=h)
        wins[f"grad{i}"] = F.Win(n.count, f32, "out")

    def launch(b):
        each = lambda kk: parr(*[b[f"{kk}{i}"] for i in range(k)])  # noqa: E731
        if form == "one":
            n = named[0][0]
            lib().nav_grad_reduce(C.byref(n.desc(b, "n0")), b["hs0"].ptr, splits, b["es0"].ptr,
                                  blocks, b["grad0"].ptr, stream())
        else:
            lib().nav_grad_reduce_multi(descs(b, *named), k, each("hs"), splits, each("es"),
                                        blocks, each("grad"), stream())
    return wins, launch, {}, pads_zero([(f"grad{i}", n) for i, (n, _) in enumerate(named)])


def pair_wins(ns, n_pairs):
    """(target, source) pairs of the soft updates: the critics' targets from the critics."""
    wins, tg, sr = {}, [], []
    for j in range(n_pairs):
        wins.update(ns[f"tc{j}"].wins(f"pt{j}", "inout", "out"))
        wins.update(ns[f"cr{j}"].wins(f"ps{j}"))
        tg.append((ns[f"tc{j}"], f"pt{j}"))
        sr.append((ns[f"cr{j}"], f"ps{j}"))
    return wins, tg, sr


def b_reduce_adam(hidden, nh, polyak, with_grads, n_pairs, blocks=19, splits=3):
    ns = nets(hidden, nh)
    named = [(ns["actor"], "n0")] if polyak else [(ns["cr0"], "n0"), (ns["cr1"], "n1")]
    k = len(named)
    wins, pads = {}, []
    for i, (n, name) in enumerate(named):
        e, h = slabs_for(n, blocks, splits, 7 + i)
        m, v = moments(n, 11 + i)
        wins.update(n.wins(name, "inout", "out"))
        wins[f"es{i}"] = F.Win(e.size, f32, "in", pitch=n.ec, init=e)
        wins[f"hs{i}"] = F.Win(h.size, f32, "in", pitch=n.hp, init=h)
        wins[f"m{i}"] = F.Win(n.count, f32, "inout", init=m)
        wins[f"v{i}"] = F.Win(n.count, f32, "inout", init=v)
        pads += [(f"{name}.p", n), (f"m{i}", n), (f"v{i}", n)]
        if with_grads:
            wins[f"grad{i}"] = F.Win(n.count, f32, "out")
            pads.append((f"grad{i}", n))
    tg = sr = own = []
    if polyak:
        wins.update(ns["atgt"].wins("own", "inout", "out"))
        own = [(ns["atgt"], "own")]
        pads.append(("own.p", ns["atgt"]))
        pw, tg, sr = pair_wins(ns, n_pairs)
        wins.update(pw)
        pads += [(f"pt{j}.p", ns[f"tc{j}"]) for j in range(n_pairs)]

    def launch(b):
        each = lambda kk: parr(*[b[f"{kk}{i}"] for i in range(k)])  # noqa: E731
        head = [descs(b, *named), k, each("hs"), splits, each("es"), blocks,
                each("grad") if with_grads else None, each("m"), each("v"),
                R.f32c(0.9), R.f32c(0.999), R.f32c(1e-8), farr(*[1e-3] * k), farr(*[0.5] * k)]
        if polyak:
            lib().nav_grad_reduce_adam_polyak(*head, descs(b, *own),
                                              descs(b, *tg) if n_pairs else None,
                                              descs(b, *sr) if n_pairs else None, n_pairs,
                                              R.f32c(0.25), stream())
        else:
            lib().nav_grad_reduce_adam(*head, stream())
    return wins, launch, {}, pads_zero(pads)


def b_adam(hidden, nh, form):
    """form: adam | adam_multi | adam_polyak_multi | polyak | polyak_multi | pack."""
    ns = nets(hidden, nh)
    wins, pads = {}, []
    if form in ("adam", "adam_multi", "adam_polyak_multi"):
        named = [(ns["actor"], "n0")] if form == "adam" else [(ns["cr0"], "n0"), (ns["cr1"], "n1")]
        for i, (n, name) in enumerate(named):
            g = np.random.default_rng(40 + i)
            m, v = moments(n, 21 + i)
            wins.update(n.wins(name, "inout", "out"))
            wins[f"grad{i}"] = F.Win(n.count, f32, "in",
                                     init=(g.standard_normal(n.count) * n.logical).astype(f32))
            wins[f"m{i}"] = F.Win(n.count, f32, "inout", init=m)
            wins[f"v{i}"] = F.Win(n.count, f32, "inout", init=v)
            pads += [(f"{name}.p", n), (f"m{i}", n), (f"v{i}", n)]
        k = len(named)
        own, tg, sr = [], [], []
        if form == "adam_polyak_multi":
            for i in range(2):
                wins.update(ns[f"tc{i}"].wins(f"own{i}", "inout", "out"))
                own.append((ns[f"tc{i}"], f"own{i}"))
                pads.append((f"own{i}.p", ns[f"tc{i}"]))
            wins.update(ns["atgt"].wins("pt0", "inout", "out"))
            wins.update(ns["actor"].wins("ps0"))
            tg, sr = [(ns["atgt"], "pt0")], [(ns["actor"], "ps0")]
            pads.append(("pt0.p", ns["atgt"]))

        def launch(b):
            each = lambda kk: parr(*[b[f"{kk}{i}"] for i in range(k)])  # noqa: E731
            b1, b2, eps = R.f32c(0.9), R.f32c(0.999), R.f32c(1e-8)
            if form == "adam":
                n = named[0][0]
                lib().nav_adam(C.byref(n.desc(b, "n0")), b["grad0"].ptr, b["m0"].ptr, b["v0"].ptr,
                               b1, b2, eps, R.f32c(1e-3), R.f32c(0.5), stream())
                return
            head = [descs(b, *named), k, each("grad"), each("m"), each("v"), b1, b2, eps,
                    farr(1e-3, 2e-3), farr(0.5, 0.25), 2.0]
            if form == "adam_multi":
                lib().nav_adam_multi(*head, stream())
            else:
                lib().nav_adam_polyak_multi(*head, descs(b, *own), descs(b, *tg), descs(b, *sr),
                                            1, R.f32c(0.25), stream())
        return wins, launch, {}, pads_zero(pads)
    if form in ("polyak", "polyak_multi"):
        pairs = [("atgt", "actor")] if form == "polyak" else \
            [("atgt", "actor"), ("tc0", "cr0"), ("tc1", "cr1")]
        tg, sr = [], []
        for j, (t, s) in enumerate(pairs):
            wins.update(ns[t].wins(f"t{j}", "inout", "out"))
            wins.update(ns[s].wins(f"s{j}"))
            tg.append((ns[t], f"t{j}"))
            sr.append((ns[s], f"s{j}"))
            pads.append((f"t{j}.p", ns[t]))

        def launch(b):
            if form == "polyak":
                lib().nav_polyak(C.byref(tg[0][0].desc(b, "t0")), C.byref(sr[0][0].desc(b, "s0")),
                                 R.f32c(0.25), stream())
            else:
                lib().nav_polyak_multi(descs(b, *tg), descs(b, *sr), len(pairs), R.f32c(0.25),
                                       stream())
        return wins, launch, {}, pads_zero(pads)
    n = ns["cr0"]
    wins.update(n.wins("n0", "in", "out"))

    def launch(b):
        lib().nav_mlp_pack(C.byref(n.desc(b, "n0")), stream())
    return wins, launch, {}, None


# ---------------------------------------------------------------- the glue
def b_replay_sample(n):
    d = data(n)
    wins = {"ring": F.Win(RING * 8, f32, "in", pitch=8, init=d["rows"]),
            "idx": F.Win(n, i64, "in", init=d["idx"]),
            "batch": F.Win(n * 8, f32, "out", pitch=8)}

    def launch(b):
        from nav._lib import NavReplay
        rd = NavReplay(b["ring"].addr, RING)
        lib().nav_replay_sample(C.byref(rd), RING, n, b["idx"].ptr, SLO, SHI, 3, b["batch"].ptr,
                                stream())
    return wins, launch, {}, None


def b_strided_copy(n):
    d = data(max(n, 2))
    src = np.resize(d["rows"], (n, 8))
    wins = {"src": F.Win(n * 8, f32, "in", pitch=8, init=src),
            "dst": F.Win(n * 6, f32, "out", pitch=6)}
    o = np.ones((n, 6), bool)
    o[:, 3:5] = False

    def launch(b):
        lib().nav_strided_copy(b["src"].ptr, 8, 2, b["dst"].ptr, 6, 3, n, 2, stream())
    return wins, launch, {"dst": o}, None


def b_fill(n):
    wins = {"x": F.Win(n, f32, "out")}

    def launch(b):
        lib().nav_fill(b["x"].ptr, n, 1.5, stream())
    return wins, launch, {}, None


def b_mix_idx(B, B_demo):
    wins = {"ic": F.Win(B, i64, "out"), "ia": F.Win(B, i64, "out")}

    def launch(b):
        lib().nav_td3_mix_idx(RING, B, B_demo, RING, 40, SLO, SHI, 3, b["ic"].ptr, b["ia"].ptr,
                              stream())
    return wins, launch, {}, None


def b_nstep_rows(B, n_step):
    d = data(B)
    g = np.random.default_rng(B + n_step)
    wins = {"ring": F.Win(RING * 8, f32, "in", pitch=8, init=d["rows"]),
            "cut": F.Win(RING, u8, "in", init=(g.random(RING) < 0.1) | (d["rows"][:, 7] != 0)),
            "idx": F.Win(B, i64, "in", init=d["idx"]),
            "staged": F.Win(B * 8, f32, "out", pitch=8),
            "steps": F.Win(B, i32, "out")}

    def launch(b):
        from nav._lib import NavReplay
        rd = NavReplay(b["ring"].addr, RING)
        lib().nav_nstep_rows(C.byref(rd), b["cut"].ptr, RING, 123, 7, n_step, 0.99, B,
                             b["idx"].ptr, SLO, SHI, 3, b["staged"].ptr, b["steps"].ptr, stream())
    return wins, launch, {}, None


def ring_window(cap, base, n, width=1):
    """Untouched: entries outside [base, base + n) modulo cap."""
    m = np.ones((cap, width), bool)
    m[(base + np.arange(n)) % cap] = False
    return m.reshape(-1)


def b_nstep_stamp(cap, pos, n):
    g = np.random.default_rng(n)
    wins = {"cut": F.Win(cap, u8, "out"),
            "flags": F.Win(n, u8, "in", init=g.integers(0, 32, n))}

    def launch(b):
        lib().nav_nstep_stamp(b["cut"].ptr, cap, pos, n, b["flags"].ptr, stream())
    return wins, launch, {"cut": ring_window(cap, pos, n)}, None


def b_per_stamp(cap, pos, n):
    nsum = lib().nav_per_sums_count(cap)
    wins = {"pri": F.Win(cap, u32, "out"),
            "sums": F.Win(nsum, np.uint64, "in", init=np.zeros(nsum, np.uint64)),
            "stat": F.Win(4, u32, "in", init=[3 * 65536, 0, 0, 0])}

    def launch(b):
        from nav._lib import NavPer
        per = NavPer(b["pri"].addr, b["sums"].addr, b["stat"].addr, cap)
        lib().nav_per_stamp(C.byref(per), pos, n, stream())
    return wins, launch, {"pri": ring_window(cap, pos, n)}, None


def b_replay_push(cap, base, n):
    g = np.random.default_rng(n + 3)
    wins = {"ring": F.Win(cap * 8, f32, "out", pitch=8)}
    for name, w in (("state", 2), ("action", 2), ("reward", 1), ("next", 2)):
        wins[name] = F.Win(n * w, f64, "in", pitch=w, init=g.standard_normal(n * w) * 10)
    wins["done"] = F.Win(n, u8, "in", init=g.integers(0, 2, n))

    def launch(b):
        from nav._lib import NavReplay
        rd = NavReplay(b["ring"].addr, cap)
        lib().nav_replay_push(C.byref(rd), base, n, b["state"].ptr, b["action"].ptr,
                              b["reward"].ptr, b["next"].ptr, b["done"].ptr, stream())
    return wins, launch, {"ring": ring_window(cap, base, n, 8)}, None


# ---------------------------------------------------------------- acting
def b_act(hidden, nh, n):
    actor = nets(hidden, nh)["actor"]
    g = np.random.default_rng(n + nh)
    wins = {"state": F.Win(n * 2, f64, "in", pitch=2, init=g.random(n * 2) * 100),
            "goal": F.Win(n * 2, f64, "in", pitch=2, init=g.random(n * 2) * 100),
            "nscale": F.Win(n, f64, "in", init=g.random(n)),
            "z": F.Win(n * 2, f64, "in", pitch=2, init=g.standard_normal(n * 2)),
            "action": F.Win(n * 2, f64, "out", pitch=2),
            "residual": F.Win(n * 2, f32, "out", pitch=2)}
    wins.update(actor.wins("actor"))

    def launch(b):
        from nav._lib import params_struct
        lib().nav_act(C.byref(params_struct()), C.byref(actor.desc(b, "actor")), n,
                      b["state"].ptr, b["goal"].ptr, b["nscale"].ptr, b["z"].ptr, 0, 0,
                      b["action"].ptr, b["residual"].ptr, stream())
    return wins, launch, {}, None


SOA = (("state", f64, 2), ("goal", f64, 2), ("region", f64, 4), ("hist", f64, 2), ("meta", u32, 1),
       ("plan_index", i32, 1), ("path_length", i32, 1), ("episodes", i32, 1),
       ("noise_scale", f64, 1))


@functools.lru_cache(maxsize=None)
def tick_state(n):
    """An initialised env set (nav_env_init, no demonstration phase) and its field, on the host."""
    import torch
    from conftest import golden
    from nav.vec_env import VecEnv, make_field
    g = golden("dynamics.npz")
    field = make_field(g["speed"], g["angle"], "cuda")
    env = VecEnv(n, field, envs_per_group=64, demo_flag=False)
    torch.cuda.synchronize()
    st = {name: getattr(env, name).cpu().numpy() for name, _, _ in SOA}
    st["field"] = field.cpu().numpy()
    return st


def b_act_tick(hidden, nh, n, cap, base):
    actor = nets(hidden, nh)["actor"]
    st = tick_state(n)
    g = np.random.default_rng(n)
    wins = {"field": F.Win(st["field"].size, f32, "in", pitch=2, init=st["field"]),
            "z": F.Win(n * 2, f64, "in", pitch=2, init=g.standard_normal(n * 2)),
            "ring": F.Win(cap * 8, f32, "out", pitch=8),
            "next_state": F.Win(n * 2, f64, "out", pitch=2),
            "goal_term": F.Win(n, f64, "out"), "flags": F.Win(n, u8, "out"),
            "block_stats": F.Win((n + 63) // 64 * 8, f32, "out", pitch=8),
            "action": F.Win(n * 2, f64, "out", pitch=2)}
    for name, dt, w in SOA:
        role = "in" if name in ("goal", "region") else "inout"
        wins["env." + name] = F.Win(st[name].size, dt, role, pitch=w, init=st[name])
    wins.update(actor.wins("actor"))

    def launch(b):
        from nav._lib import NavEnvSoa, NavReplay, NavStepOut, params_struct
        soa = NavEnvSoa(n, *[b["env." + name].addr for name, _, _ in SOA])
        out = NavStepOut(b["next_state"].addr, b["goal_term"].addr, b["flags"].addr,
                         b["block_stats"].addr)
        rd = NavReplay(b["ring"].addr, cap)
        lib().nav_act_tick(C.byref(params_struct(seed_lo=SLO, seed_hi=SHI)),
                           C.byref(actor.desc(b, "actor")), C.byref(soa), b["field"].ptr,
                           b["z"].ptr, 5, 0, C.byref(rd), base, C.byref(out), None, None, 64,
                           None, None, b["action"].ptr, None, stream())
    return wins, launch, {"ring": ring_window(cap, base, n, 8)}, None


# ---------------------------------------------------------------- population forms
POP_SHAPE, POP_B, POP_P, POP_TAIL = (64, 2), 100, 3, 40
# every array of a member: field -> (window name, dtype, elements, pitch); built in pop_fields
POP_OUT = {
    "critic_rows": ["batch", "dq0", "dq1", "lp0", "lp1", "es0", "es1", "acts0", "acts1", "dz0",
                    "dz1", "masks0", "masks1"],
    "actor_rows": ["batch_actor", "q", "da", "acts_actor", "dz_actor", "masks_actor", "masks0",
                   "es_actor"],
    "actor_rows_bc": ["batch_actor", "q", "da", "acts_actor", "dz_actor", "masks_actor", "masks0",
                      "es_actor", "bc_part"],
    "wgrad": ["hs0", "hs1"],
    "reduce_adam": ["grad0", "grad1"],
    "mix_idx": ["idx_c", "idx_a"],
}


def pop_member_arrays(m):
    """Member m's arrays after its own critic and actor rows, name -> host array."""
    hidden, nh = POP_SHAPE
    ns = nets(hidden, nh)
    c, a, d = (critic_state(hidden, nh, POP_B, m + 1), actor_state(hidden, nh, POP_B, m + 1),
               data(POP_B, m + 1))
    g = np.random.default_rng(500 + m)
    cr, ac = ns["cr0"], ns["actor"]
    splits = 2
    x = {"ring": np.concatenate([d["rows"], (g.standard_normal((POP_TAIL, 8)) * 10).astype(f32)]),
         "idx_c": d["idx"], "idx_a": d["idx_a"], "eps": d["eps"],
         "batch": c["batch"], "batch_actor": a["batch"], "q": a["q"], "da": a["da"],
         "acts_actor": a["acts"], "dz_actor": a["dz"], "masks_actor": a["ma"], "es_actor": a["es"],
         "bc_part": np.zeros(lib().nav_mlp_row_blocks(POP_B), f32),
         "grad_actor": np.zeros(ac.count, f32)}
    x["m_actor"], x["v_actor"] = moments(ac, 70 + m)
    for i in range(2):
        for k in ("dq", "lp", "es", "acts", "dz", "masks"):
            x[f"{k}{i}"] = c[f"{k}{i}"]
        x[f"hs{i}"] = slabs_for(cr, 1, splits, 900 + 10 * m + i)[1]
        x[f"grad{i}"] = np.zeros(cr.count, f32)
        x[f"m{i}"], x[f"v{i}"] = moments(cr, 80 + 2 * m + i)
    return x


PITCH = {"ring": 8, "batch": 8, "batch_actor": 8, "eps": 2, "da": 2}


def b_pop(entry):
    from nav._lib import NavReplay, NavTd3Member, NavTd3MemberBc
    hidden, nh = POP_SHAPE
    ns = nets(hidden, nh)
    B, P = POP_B, POP_P
    splits = 2
    net_names = ["actor", "cr0", "cr1", "ta", "tc0", "tc1"]
    written_nets = ["cr0", "cr1"] if entry == "reduce_adam" else []
    inout = ["m0", "v0", "m1", "v1"] if entry == "reduce_adam" else []
    wins, unt, pads = {}, {}, []
    for m in range(P):
        x = pop_member_arrays(m)
        for name, arr in x.items():
            pitch = PITCH.get(name)
            if name.startswith(("acts", "dz", "hs")):
                pitch = pad32(hidden)
            elif name.startswith("masks"):
                pitch = pad32(hidden) // 32 * 64
            elif name.startswith("es"):
                pitch = (ns["actor"] if name == "es_actor" else ns["cr0"]).ec
            role = "out" if name in POP_OUT[entry] else "inout" if name in inout else "in"
            wins[f"{m}.{name}"] = F.Win(arr.size, arr.dtype, role, pitch=pitch,
                                        init=None if role == "out" else arr)
        for nn in net_names:
            if nn in written_nets:
                wins.update(ns[nn].wins(f"{m}.{nn}", "inout", "out"))
                pads.append((f"{m}.{nn}.p", ns[nn]))
            else:
                wins.update(ns[nn].wins(f"{m}.{nn}"))
        if entry == "reduce_adam":
            pads += [(f"{m}.{k}{i}", ns["cr0"]) for k in ("grad", "m", "v") for i in range(2)]
        mid = mid_of(nh)
        for name in POP_OUT[entry]:
            if name.startswith(("acts", "dz")):
                unt[f"{m}.{name}"] = layers_untouched(nh, B, pad32(hidden), mid)
            elif name.startswith("masks"):
                unt[f"{m}.{name}"] = mask_untouched(pad32(hidden), nh, B)

    def launch(b):
        members = (NavTd3Member * P)()
        bcs = (NavTd3MemberBc * P)()
        for m in range(P):
            t = members[m]
            a = lambda name: b[f"{m}.{name}"].addr  # noqa: E731
            t.actor, t.target_actor = ns["actor"].desc(b, f"{m}.actor"), ns["ta"].desc(b, f"{m}.ta")
            for i in range(2):
                t.critics[i] = ns[f"cr{i}"].desc(b, f"{m}.cr{i}")
                t.target_critics[i] = ns[f"tc{i}"].desc(b, f"{m}.tc{i}")
                t.m_critic[i], t.v_critic[i] = a(f"m{i}"), a(f"v{i}")
                t.dq[i], t.loss_part[i], t.edge_slabs[i] = a(f"dq{i}"), a(f"lp{i}"), a(f"es{i}")
                t.acts[i], t.dz[i], t.masks[i] = a(f"acts{i}"), a(f"dz{i}"), a(f"masks{i}")
                t.hidden_slabs[i], t.grad_critic[i] = a(f"hs{i}"), a(f"grad{i}")
            t.replay = NavReplay(a("ring"), RING)
            t.m_actor, t.v_actor = a("m_actor"), a("v_actor")
            t.actor_lr, t.critic_lr = 1e-4 * (m + 1), 1e-3 * (m + 1)
            t.policy_noise, t.noise_clip, t.max_action, t.gamma, t.tau = 0.2, 0.5, 5.0, 0.99, 0.25
            t.seed_lo, t.seed_hi = SLO + m, SHI
            t.idx_critic, t.idx_actor, t.eps = a("idx_c"), a("idx_a"), a("eps")
            t.batch, t.batch_actor = a("batch"), a("batch_actor")
            t.edge_slabs_actor, t.acts_actor = a("es_actor"), a("acts_actor")
            t.dz_actor, t.masks_actor = a("dz_actor"), a("masks_actor")
            t.q, t.da, t.grad_actor = a("q"), a("da"), a("grad_actor")
            bcs[m] = NavTd3MemberBc(7 * m, POP_TAIL, 1.0, 0.5 if m else 0.0, a("idx_c"), a("idx_a"),
                                    a("bc_part"))
        L, s = lib(), stream()
        table, tp = device_table(L.nav_td3_pop_table_bytes(P))
        bct, bp = device_table(L.nav_td3_pop_bc_table_bytes(P))
        L.nav_td3_pop_table_build(members, P, B, splits, splits, tp, s)
        if entry == "critic_rows":
            L.nav_td3_critic_rows_pop(members, P, B, tp, RING, 3, -1, s)
        elif entry == "actor_rows":
            L.nav_td3_actor_rows_pop(members, P, B, tp, RING, 3, s)
        elif entry == "wgrad":
            L.nav_mlp_wgrad_pop(members, P, B, tp, 0, splits, s)
        elif entry == "reduce_adam":
            L.nav_grad_reduce_adam_pop(members, P, B, tp, 0, R.f32c(0.9), R.f32c(0.999),
                                       R.f32c(1e-8), 0.1, R.f32c(0.5), 0, s)
        else:
            L.nav_td3_pop_bc_table_build(members, bcs, P, B, bp, s)
            if entry == "mix_idx":
                L.nav_td3_mix_idx_pop(members, bcs, P, B, bp, RING, 3, 1, s)
            else:
                L.nav_td3_actor_rows_bc_pop(members, bcs, P, B, bp, RING, 3, s)
        b["0.ring"].mem.sync()  # the tables live until the launch is done
    return wins, launch, unt, pads_zero(pads) if pads else None


# ---------------------------------------------------------------- the table
for _shape in SHAPES:
    _h, _nh = _shape
    _s = f"{_h}x{_nh}"
    for _M in rows_of(_shape):
        _t = f"{_s}-{_M}"
        _sub = 1 << (_nh - 1) if _nh > 1 else 0
        case(f"forward-actor-1net-target-ld8col5-savesub-{_t}", b_forward, hidden=_h, nh=_nh, M=_M,
             kind="actor", n_nets=1, out_mode=1, ld_out=8, out_col=5, save_mask=_sub)
        case(f"forward-critic-2nets-plain-saveall-{_t}", b_forward, hidden=_h, nh=_nh, M=_M,
             kind="critic", n_nets=2, out_mode=0, ld_out=1, out_col=0, save_mask=(1 << _nh) - 1)
        case(f"critic_forward-{_t}", b_critic_forward, hidden=_h, nh=_nh, B=_M)
        case(f"backward-critic-dx-savesub-{_t}", b_backward, hidden=_h, nh=_nh, M=_M,
             kind="critic", dx=True, h_top=False, save_mask=1)
        case(f"backward-actor-nodx-htop-saveall-{_t}", b_backward, hidden=_h, nh=_nh, M=_M,
             kind="actor", dx=False, h_top=True, save_mask=(1 << _nh) - 1)
        if _nh > 1:
            case(f"wgrad-critic-libsplits-{_t}", b_wgrad, hidden=_h, nh=_nh, B=_M, group="critic",
                 splits=0)
            case(f"wgrad-critic-1split-{_t}", b_wgrad, hidden=_h, nh=_nh, B=_M, group="critic",
                 splits=1)
            case(f"wgrad-actor-libsplits-{_t}", b_wgrad, hidden=_h, nh=_nh, B=_M, group="actor",
                 splits=0)
            if _M in (33, 100):
                case(f"wgrad-critic-5splits-{_t}", b_wgrad, hidden=_h, nh=_nh, B=_M,
                     group="critic", splits=5)
                case(f"wgrad-actor-5splits-{_t}", b_wgrad, hidden=_h, nh=_nh, B=_M, group="actor",
                     splits=5)
        for _rb in (0, 1):
            for _tw in (0, 1):
                case(f"critic_rows-rb{_rb}-twins{_tw}-{_t}", b_critic_rows, hidden=_h, nh=_nh,
                     B=_M, row_backward=_rb, split_twins=_tw)
        case(f"critic_rows_w-{_t}", b_critic_rows, hidden=_h, nh=_nh, B=_M, row_backward=1,
             split_twins=-1, weighted=True)
        case(f"actor_rows-{_t}", b_actor_rows, hidden=_h, nh=_nh, B=_M)
        for _bd in sorted({0, min(7, _M), _M}):
            case(f"actor_rows_bc-demo{_bd}-{_t}", b_actor_rows, hidden=_h, nh=_nh, B=_M, form="bc",
                 B_demo=_bd)
        case(f"actor_rows_bc-nocritic-{_t}", b_actor_rows, hidden=_h, nh=_nh, B=_M, form="bc",
             B_demo=min(7, _M), critic=False)
        case(f"actor_rows_bcq-qdemo-{_t}", b_actor_rows, hidden=_h, nh=_nh, B=_M, form="bcq",
             B_demo=min(7, _M))
        case(f"actor_rows_bcq-noqdemo-{_t}", b_actor_rows, hidden=_h, nh=_nh, B=_M, form="bcq",
             B_demo=min(7, _M), q_demo=False)
    for _blocks in (1, 19, 256, 257, 600):
        case(f"grad_reduce-{_s}-blocks{_blocks}", b_reduce, hidden=_h, nh=_nh, blocks=_blocks,
             form="one")
        case(f"grad_reduce_multi-{_s}-blocks{_blocks}", b_reduce, hidden=_h, nh=_nh,
             blocks=_blocks, form="multi")
    for _g in (True, False):
        case(f"grad_reduce_adam-{_s}-grads{int(_g)}", b_reduce_adam, hidden=_h, nh=_nh,
             polyak=False, with_grads=_g, n_pairs=0)
        for _np in (0, 2):
            case(f"grad_reduce_adam_polyak-{_s}-grads{int(_g)}-pairs{_np}", b_reduce_adam,
                 hidden=_h, nh=_nh, polyak=True, with_grads=_g, n_pairs=_np)
    for _f in ("adam", "adam_multi", "adam_polyak_multi", "polyak", "polyak_multi"):
        case(f"{_f}-{_s}", b_adam, hidden=_h, nh=_nh, form=_f)
    if _nh > 1:
        case(f"mlp_pack-{_s}", b_adam, hidden=_h, nh=_nh, form="pack")
    for _n in (1, 97):
        case(f"act-{_s}-{_n}", b_act, hidden=_h, nh=_nh, n=_n)
    for _n in (64, 192):
        case(f"act_tick-{_s}-{_n}", b_act_tick, hidden=_h, nh=_nh, n=_n, cap=256, base=256 - 40)
for _n in (1, 255, 257):
    case(f"replay_sample-{_n}", b_replay_sample, n=_n)
    case(f"strided_copy-{_n}", b_strided_copy, n=_n)
    case(f"fill-{_n}", b_fill, n=_n)
case("mix_idx-100-demo7", b_mix_idx, B=100, B_demo=7)
case("mix_idx-257-demo0", b_mix_idx, B=257, B_demo=0)
for _k in (1, 16):
    case(f"nstep_rows-nstep{_k}", b_nstep_rows, B=100, n_step=_k)
case("nstep_stamp-wraps", b_nstep_stamp, cap=500, pos=480, n=64)
case("per_stamp-wraps", b_per_stamp, cap=500, pos=480, n=64)
case("replay_push-wraps", b_replay_push, cap=500, base=480, n=64)
for _e in POP_OUT:
    case(f"pop-{_e}-64x2-100-3members", b_pop, entry=_e)


@pytest.fixture(scope="module")
def nav():
    from nav import _lib
    _lib.require_gpu()
    return _lib.lib()


@pytest.mark.parametrize("fn,kw", CASES)
def test_footprint(nav, request, fn, kw):
    """The five checks of tests/footprint.py on one launch (and +0.0 on every padded slot after
    an optimizer step)."""
    t0 = time.perf_counter()
    wins, launch, untouched, post = fn(**kw)
    t1 = time.perf_counter()
    findings, vals = F.check(launch, wins, untouched, collect=True)
    if post:
        findings += post(vals)
    t2 = time.perf_counter()
    print(f"{request.node.callspec.id}: build {t1 - t0:.3f} s, check {t2 - t1:.3f} s")
    path = os.environ.get("NAV_FOOTPRINT_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(f"{request.node.callspec.id}\t{t1 - t0:.3f}\t{t2 - t1:.3f}\t{findings}\n")
    assert not findings, findings


def test_device_checker_sees_a_stray_and_a_skipped_store(nav):
    """The device backend of the checker on a launch that is wrong by one element: nav_fill asked
    for n + 1 elements of an n-element window stores into the guard (check 1, and the
    zero-allocation run is then not made); asked for n - 1 it leaves the last element (check 3)."""
    n = 257
    for count, cause in ((n + 1, F.STRAY), (n - 1, F.SKIPPED)):
        findings, _ = F.check(lambda b: lib().nav_fill(b["x"].ptr, count, 1.5, stream()),
                              {"x": F.Win(n, f32, "out")}, collect=True)
        assert {c for c, _ in findings} == {cause}, findings
        assert str(n if cause == F.STRAY else n - 1) in findings[0][1]
