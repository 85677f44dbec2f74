"""The fused learner launches of the GPU tests, stated once: nav_td3_critic_rows(_w),
nav_td3_actor_rows(_bc, _bcq) and the nav_mlp_wgrad -> nav_grad_reduce tail behind them.

Every entry point is called through abi_args.by_name: the keywords are include/navenv.h's
parameter names, checked against the header in order, and the status must be 0. The argument
order of an entry point appears here and nowhere else in the tests.

The caller chooses the prefill of the outputs (`fill`: NaN or 0.0), because the prefill is part of
what it asserts: a layer the launch does not save stays NaN, a NULL output is left alone. The ReLU
mask buffers are the nets' own mask_buffer()s; keep_part is prefilled with -1.

One set of output keys. Critic launches (lists of two, one per online critic): batch, dq, lp
[2][row blocks], es, acts, dz, masks, td (the weighted form only), nblk. Actor launches: batch,
q, da, acts, dz, ma, mc, es, nblk, part (the BC forms), q_demo and keep_part (the Q-filter).
wgrad() adds hs and splits."""
import ctypes as C

import torch

import mlp_ref as R
from abi_args import by_name

DEV = R.DEV
SEED = 1707366464
SLO, SHI = SEED & 0xFFFFFFFF, SEED >> 32
ACTOR, CRITIC = (2, 2), (4, 1)  # (d_in, d_out)
# the nets of mlp_ref.epoch_case (bc_ref.bc_case, bcq_ref.bcq_case: actor and cr0) by name
KIND = dict(ta=ACTOR, actor=ACTOR, atgt=ACTOR, tc0=CRITIC, tc1=CRITIC, cr0=CRITIC, cr1=CRITIC)


def full(fill, *shape):
    return torch.full(shape, fill, device=DEV)


def nan(*shape):
    return full(float("nan"), *shape)


def device_net(layers, d_in, d_out, hidden, nh):
    from nav.mlp import DeviceMLP
    return DeviceMLP(d_in, d_out, hidden, nh, DEV).load([(W.numpy(), b.numpy()) for W, b in layers])


def device_epoch(case):
    """(nets, dev) of an mlp_ref.epoch_case, a bc_ref.bc_case or a bcq_ref.bcq_case: every net of
    the case on the device by name, the rows, the injected indices and noise the case has, and the
    ring descriptor over the case's ring size (a BC case's demonstration tail lies behind it)."""
    from nav._lib import NavReplay
    nets = {name: device_net(layers, *KIND[name], case["hidden"], case["nh"])
            for name, layers in case["layers"].items()}
    dev = {k: case[k].to(DEV).contiguous() for k in ("rows", "idx", "idx_a", "eps") if k in case}
    dev["size"] = case["ring"]
    dev["rd"] = NavReplay(dev["rows"].data_ptr(), dev["size"])
    return nets, dev


def _raw():
    from nav._lib import lib
    return lib().raw


def critic_rows(nets, dev, B, *, fill, split=-1, row_backward=1, save=True, w=None, counter=3,
                size=None, rd=None, gamma=0.99):
    """nav_td3_critic_rows, or nav_td3_critic_rows_w with the row weights `w`, of nets ta, tc0,
    tc1, cr0, cr1 on dev's ring (or rd / size), indices dev["idx"] and noise dev["eps"] (either
    may be None: the kernel's own draw), with each online critic's middle layers saved and its dz
    buffers bound (save=False: no acts, no dz)."""
    from nav._lib import descs, lib, parr, ptr, stream_handle
    L = lib()
    cr = [nets["cr0"], nets["cr1"]]
    hp, nh = cr[0].hp, cr[0].n_hidden
    mid = cr[0].middle_layers() if save else 0
    nblk = L.nav_mlp_row_blocks(B)
    ec = L.nav_mlp_edge_count(4, 1, hp, nh)
    two = lambda *shape: [full(fill, *shape), full(fill, *shape)]  # noqa: E731
    o = dict(batch=full(fill, B, 8), dq=two(B), lp=full(fill, 2, nblk), es=two(nblk, ec),
             masks=[c.mask_buffer(B) for c in cr], nblk=nblk)
    if save:
        o.update(acts=two(nh, B, hp), dz=two(nh, B, hp))
    args = dict(
        target_actor=C.byref(nets["ta"].desc()), target_critics=descs(nets["tc0"], nets["tc1"]),
        critics=descs(*cr), replay=C.byref(dev["rd"] if rd is None else rd),
        size=dev["size"] if size is None else size, B=B, idx=ptr(dev["idx"]), seed_lo=SLO,
        seed_hi=SHI, counter=counter, eps=ptr(dev["eps"]), policy_noise=0.2, noise_clip=0.5,
        max_action=5.0, gamma=gamma, batch=ptr(o["batch"]), dq=parr(*o["dq"]),
        loss_part=parr(o["lp"][0], o["lp"][1]), edge_slabs=parr(*o["es"]),
        acts=parr(*o["acts"]) if save else None, save_mask=mid, masks=parr(*o["masks"]),
        row_backward=row_backward, dz=parr(*o["dz"]) if save else None, dz_save_mask=mid,
        split_twins=split)
    if w is None:
        by_name(L.raw, "nav_td3_critic_rows", **args, stream=stream_handle())
    else:
        o["td"] = [nan(B), nan(B)]
        by_name(L.raw, "nav_td3_critic_rows_w", **args, w=ptr(w), td_abs=parr(*o["td"]),
                stream=stream_handle())
    return o


def actor_rows(nets, dev, B, *, form, fill, b_demo=0, q_weight=1.0, bc_weight=0.0, critic=True,
               save=True, save_mask=None, counter=3):
    """nav_td3_actor_rows (form "plain"), nav_td3_actor_rows_bc ("bc") or nav_td3_actor_rows_bcq
    ("bcq") of nets actor and cr0 on dev's ring and dev["idx_a"] (None: the kernel's own draw).
    critic=False is the BC form's pure-BC launch: critic, q and masks_critic NULL. save_mask: the
    actor's saved layers (its middle layers unless given); save=False binds no q, acts or dz."""
    from nav._lib import lib, ptr, stream_handle
    L = lib()
    actor, cr = nets["actor"], nets["cr0"]
    hp, nh = actor.hp, actor.n_hidden
    mid = actor.middle_layers() if save else 0
    nblk = L.nav_mlp_row_blocks(B)
    o = dict(batch=full(fill, B, 8), q=full(fill, B), da=full(fill, B, 2), ma=actor.mask_buffer(B),
             mc=cr.mask_buffer(B), es=full(fill, nblk, L.nav_mlp_edge_count(2, 2, hp, nh)),
             nblk=nblk)
    if save:
        o.update(acts=full(fill, nh, B, hp), dz=full(fill, nh, B, hp))
    args = dict(actor=C.byref(actor.desc()), critic=C.byref(cr.desc()) if critic else None,
                replay=C.byref(dev["rd"]), size=dev["size"], B=B, idx=ptr(dev["idx_a"]),
                seed_lo=SLO, seed_hi=SHI, counter=counter)
    if form != "plain":
        o["part"] = full(fill, nblk)
        args.update(B_demo=b_demo, q_weight=q_weight, bc_weight=bc_weight)
    args.update(batch=ptr(o["batch"]), q=ptr(o["q"]) if critic and save else None, da=ptr(o["da"]))
    if form != "plain":
        args.update(bc_part=ptr(o["part"]))
    if form == "bcq":
        o.update(q_demo=full(fill, B),
                 keep_part=torch.full((nblk,), -1, dtype=torch.int32, device=DEV))
        args.update(q_demo=ptr(o["q_demo"]), keep_part=ptr(o["keep_part"]))
    args.update(acts=ptr(o["acts"]) if save else None,
                save_mask=mid if save_mask is None else save_mask,
                dz=ptr(o["dz"]) if save else None, dz_save_mask=mid, masks_actor=ptr(o["ma"]),
                masks_critic=ptr(o["mc"]) if critic else None, edge_slabs=ptr(o["es"]),
                stream=stream_handle())
    by_name(L.raw, {"plain": "nav_td3_actor_rows", "bc": "nav_td3_actor_rows_bc",
                    "bcq": "nav_td3_actor_rows_bcq"}[form], **args)
    return o


def _group(o):
    """(acts, dz, dy, ld_dy, masks, es) of a rows launch's outputs as lists, one entry per net."""
    if "da" in o:
        return [o["acts"]], [o["dz"]], [o["da"]], 2, [o["ma"]], [o["es"]]
    return o["acts"], o["dz"], o["dq"], 1, o["masks"], o["es"]


def wgrad(group, o, *, splits=None, fill):
    """nav_mlp_wgrad of the group a rows launch trained ([cr0, cr1] or [actor]) on that launch's
    outputs `o`, at `splits` (None: nav_mlp_wgrad_splits) into `fill`-prefilled hidden slabs;
    o["hs"] and o["splits"] are the reduce's inputs."""
    from nav._lib import descs, lib, parr, ptr, stream_handle
    L = lib()
    hp, nh, n = group[0].hp, group[0].n_hidden, len(group)
    B = o["batch"].shape[0]
    acts, dz, dy, ld_dy, masks, _ = _group(o)
    if splits is None:
        splits = int(L.nav_mlp_wgrad_splits(n, ld_dy, hp, nh, B))
    o["splits"] = splits
    o["hs"] = [full(fill, splits, max(4, L.nav_mlp_hidden_count(hp, nh))) for _ in group]
    by_name(L.raw, "nav_mlp_wgrad", nets=descs(*group), n_nets=n, M=B, inp=ptr(o["batch"]),
            ld_in=8, in_col=0, acts=parr(*acts), dz=parr(*dz), dy=parr(*dy), ld_dy=ld_dy,
            masks=parr(*masks), slabs=parr(*o["hs"]), splits=splits, stream=stream_handle())
    return o


def flat_grads(group, o, *, splits=None, fill):
    """wgrad(), then nav_grad_reduce per net into a NaN-prefilled flat gradient: the group's flat
    gradients, in its order."""
    from nav._lib import lib, ptr, stream_handle
    wgrad(group, o, splits=splits, fill=fill)
    es = _group(o)[5]
    out = []
    for k, net in enumerate(group):
        g = nan(net.count)
        by_name(lib().raw, "nav_grad_reduce", net=C.byref(net.desc()), hidden_slabs=ptr(o["hs"][k]),
                splits=o["splits"], edge_slabs=ptr(es[k]), edge_blocks=o["nblk"], grad=ptr(g),
                stream=stream_handle())
        out.append(g)
    return out
