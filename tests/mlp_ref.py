"""References shared by the MLP kernel tests (test code only, no fixtures).

The fp64 reference of the row kernels and the learner: one chain evaluation (`mlp_forward` /
`mlp_backward` / `mlp_chain`, and the TD3 epochs `critic_epoch` / `actor_epoch` built on it) at a
given dtype with injected ReLU decisions. The same code yields the fp64 reference, `e32` (the
error of an fp32 torch-CPU evaluation of the same chain against it) and, with `narrow=True`, a
16-bit-mantissa evaluation that stands in for a deliberately narrowed GEMM. The device's error is
measured against the same fp64 result by the callers.

Bars (`bar`): the project's fp64 bars of test_split_gemm_f32_accuracy_vs_fp64, max |err| / max
|ref| <= 2e-6 for row quantities and <= 1e-5 for cross-row sums, each widened to 8 * e32 where
fp32 itself is worse than base / 8 (cancellation in one-row batches and 8-layer chains). The
factor 8 is derived: the split keeps 22 significant bits per operand against fp32's 24 (4 x), and
the A-operand scale is per 32-row tile, so rows below their tile's maximum lose more (2 x).

ReLU kinks (`relu_band`): backward references use the kernel's own bit image (`relu_bits`); the
bits must equal the fp64 signs wherever |z| > fan_in * 1.2e-7 * (|h| @ |W|^T + |b|), and at most
max(2, 5e-4 * entries) entries of a case may lie inside that band (`assert_band_cap`)."""
import ctypes as C

import torch

DEV = "cuda"
ROW_BAR, SUM_BAR, E32_FACTOR = 2e-6, 1e-5, 8.0


def torch_mlp(layers, x):
    h = x
    for i, (W, b) in enumerate(layers):
        h = torch.nn.functional.linear(h, W, b)
        if i < len(layers) - 1:
            h = torch.relu(h)
    return h


def make_net(d_in, d_out, hidden, nh, seed):
    from nav.mlp import DeviceMLP
    from oracle.td3_oracle import make_mlp_params
    p = make_mlp_params(seed, [d_in] + [hidden] * nh + [d_out])
    net = DeviceMLP(d_in, d_out, hidden, nh, DEV).load(p)
    return net, [(torch.tensor(W), torch.tensor(b)) for W, b in p]


def _grad_flat_vs_autograd(net, tl, gflat, d_in, d_out, nh):
    from nav.mlp import layer_offsets
    offs, _ = layer_offsets(d_in, d_out, net.hp, nh)
    for l, ((W, b), (w_off, b_off, fo, fi)) in enumerate(zip(tl, offs)):
        o, i = W.shape
        gW = gflat[w_off:w_off + fo * fi].view(fo, fi)
        tol = 1e-5 * (W.grad.abs().max() + 1e-6)
        assert torch.allclose(gW[:o, :i], W.grad, rtol=1e-3, atol=tol), l
        assert (gW[o:, :] == 0).all() and (gW[:, i:] == 0).all()
        gb = gflat[b_off:b_off + o]
        assert torch.allclose(gb, b.grad, rtol=1e-3, atol=1e-5 * (b.grad.abs().max() + 1e-6)), l
        assert (gflat[b_off + o:b_off + fo] == 0).all()


def relu_bits(masks, nh, hp, hidden, M):
    """The forward's ReLU bit image ([nh][M / 32 row tiles][hp / 32][64 lanes] u16 words, C
    layout: bit i of lane (l32, h) = row (i & 3) + 8 (i >> 2) + 4 h of the tile, column l32) as
    [nh][M][hidden] booleans."""
    nt = hp // 32
    w = masks.cpu().to(torch.int32) & 0xFFFF
    n_rt = w.numel() // (nh * nt * 64)
    bits = ((w.view(nh, n_rt, nt, 2, 32, 1) >> torch.arange(16)) & 1).bool()
    r = torch.arange(32)
    hh, ii = (r >> 2) & 1, (r & 3) + 4 * (r >> 3)  # lane half and element of tile row r
    b = bits.permute(0, 1, 3, 5, 2, 4)[:, :, hh, ii]  # [nh][n_rt][32 rows][nt][32 cols]
    return b.reshape(nh, n_rt * 32, nt * 32)[:, :M, :hidden]


# ---- one chain evaluation at a given dtype ----
def narrow16(t):
    """t rounded to 16 significant bits: the two-plane bf16 split hi + lo (a 16-bit-mantissa
    operand, narrower than the kernels' 22 bits and than fp32's 24)."""
    hi = t.float().bfloat16().float()
    return (hi + (t.float() - hi).bfloat16().float()).to(t.dtype)


def _mm(a, b, narrow):
    return narrow16(a) @ narrow16(b) if narrow else a @ b


def mlp_forward(layers, x, dtype=torch.float64, narrow=False):
    """The forward of the f32 weights `layers` on rows x at `dtype` (narrow: every product's
    operands rounded to 16 significant bits). Returns (out, zs, hs): the output, every hidden
    pre-activation z_l and the layer inputs hs[l] (hs[0] = x, hs[l + 1] = relu(z_l))."""
    h, zs, hs = x.to(dtype), [], []
    for i, (W, b) in enumerate(layers):
        hs.append(h)
        if narrow:
            z = _mm(h, W.to(dtype).t(), True) + b.to(dtype)
        else:
            z = torch.nn.functional.linear(h, W.to(dtype), b.to(dtype))
        if i < len(layers) - 1:
            zs.append(z)
            h = torch.relu(z)
        else:
            h = z
    return h, zs, hs


def mlp_backward(layers, hs, dy, bits, dtype=torch.float64, narrow=False):
    """The row backward and the parameter gradients of mlp_forward's chain for dL/dy rows `dy`,
    with the injected ReLU decisions bits [nh][M][hidden]: dz[l] = dL/dz_l, dx = dL/dx, grads[l] =
    (dL/dW_l, dL/db_l) for l = 0 .. nh (the cross-row sums dz_l^T h_{l-1} and sum_rows dz_l)."""
    nh = len(layers) - 1
    g = dy.to(dtype)
    dz, grads = [None] * nh, [None] * (nh + 1)
    for l in range(nh, -1, -1):
        if l < nh:
            g = g * bits[l].to(dtype)
            dz[l] = g
        grads[l] = (_mm(g.t(), hs[l], narrow), g.sum(0))
        g = _mm(g, layers[l][0].to(dtype), narrow)
    return dz, g, grads


def mlp_chain(layers, x, dy, bits, dtype=torch.float64, narrow=False):
    """mlp_forward then mlp_backward: dict(out, z, h (the nh post-ReLU activations), dz, dx,
    grads)."""
    out, zs, hs = mlp_forward(layers, x, dtype, narrow)
    dz, dx, grads = mlp_backward(layers, hs, dy, bits, dtype, narrow)
    return dict(out=out, z=zs, h=hs[1:], dz=dz, dx=dx, grads=grads)


def _f64_forward(layers, x):
    """fp64 forward of the same f32 weights; returns the output and every hidden pre-activation."""
    out, zs, _ = mlp_forward(layers, x)
    return out, zs


def relu_band(layers, x, zs, bits, extra0=None):
    """The ReLU bits against the fp64 signs of zs (mlp_forward's, inputs x): equal wherever |z_l|
    > fan_in * 1.2e-7 * (|h_{l-1}| @ |W_l|^T + |b_l|) (asserted). extra0 [M][hidden] widens layer
    0's band where x itself is a computed quantity. Returns (entries inside the band, entries)."""
    h, inside, entries = x.double(), 0, 0
    for l, z in enumerate(zs):
        W, b = layers[l]
        band = W.shape[1] * 1.2e-7 * (h.abs() @ W.double().abs().t() + b.double().abs())
        if l == 0 and extra0 is not None:
            band = band + extra0
        outside = z.abs() > band
        assert torch.equal(bits[l][outside], (z > 0)[outside]), l
        inside += int((~outside).sum())
        entries += z.numel()
        h = torch.relu(z)
    return inside, entries


def assert_band_cap(inside, entries):
    assert inside <= max(2, 5e-4 * entries), (inside, entries)


def rel_err(got, ref):
    """max |got - ref| / max |ref| (0 / 0 = 0: an all-zero reference must be met exactly)."""
    ref = ref.double()
    err = float((got.double() - ref).abs().max())
    scale = float(ref.abs().max())
    if not err == err:
        return float("inf")
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


def bar(name, e32):
    """The bar of quantity `name`: cross-row sums (gradient tensors `dW*` / `db*`, `loss`) 1e-5,
    row quantities 2e-6, each at least 8 * e32."""
    base = SUM_BAR if name.startswith(("dW", "db", "loss")) else ROW_BAR
    return max(base, E32_FACTOR * e32)


def grad_names(nh):
    return [n for l in range(nh + 1) for n in (f"dW{l}", f"db{l}")]


def _r4(x):
    return (x + 3) // 4 * 4


def layer_offsets(d_in, d_out, hp, n_hidden):
    """nav.mlp.layer_offsets (the flat layout of include/navenv.h nav_mlp), restated so that the
    reference needs no library."""
    offs, o = [], 0
    for l in range(n_hidden + 1):
        fi = d_in if l == 0 else hp
        fo = d_out if l == n_hidden else hp
        w = o
        o += _r4(fi * fo)
        b = o
        o += _r4(fo)
        offs.append((w, b, fo, fi))
    return offs, o


def logical_mask(d_in, d_out, hidden, hp, nh):
    """[param_count] booleans: the flat layout's entries that hold a logical weight or bias (the
    rest: padded rows and columns and the segments' rounding slots)."""
    offs, count = layer_offsets(d_in, d_out, hp, nh)
    sizes = [d_in] + [hidden] * nh + [d_out]
    used = torch.zeros(count, dtype=torch.bool)
    for l, (w_off, b_off, fo, fi) in enumerate(offs):
        used[w_off:w_off + fo * fi].view(fo, fi)[:sizes[l + 1], :sizes[l]] = True
        used[b_off:b_off + sizes[l + 1]] = True
    return used


def flat_grad_tensors(gflat, d_in, d_out, hidden, hp, nh):
    """The flat device-layout gradient as {dW0, db0, ...} at logical sizes; every padded row,
    column and rounding slot must be exactly 0 and every entry finite (NaN-prefilled buffers)."""
    offs, count = layer_offsets(d_in, d_out, hp, nh)
    assert gflat.numel() == count and bool(torch.isfinite(gflat).all())
    assert bool((gflat[~logical_mask(d_in, d_out, hidden, hp, nh)] == 0).all())
    sizes = [d_in] + [hidden] * nh + [d_out]
    out = {}
    for l, (w_off, b_off, fo, fi) in enumerate(offs):
        o, i = sizes[l + 1], sizes[l]
        out[f"dW{l}"] = gflat[w_off:w_off + fo * fi].view(fo, fi)[:o, :i]
        out[f"db{l}"] = gflat[b_off:b_off + o]
    return out


def compare(dev, ref, f32, scales=None):
    """[(name, err, e32, bar)] for every quantity of ref: the device's and the fp32 chain's max
    |x - ref| / scale against the fp64 chain, scale = max |ref| (or scales[name])."""
    out = []
    for n, r in ref.items():
        if scales and n in scales:
            sc = scales[n]
            err = float((dev[n].double() - r.double()).abs().max()) / sc
            e32 = float((f32[n].double() - r.double()).abs().max()) / sc
            err = err if err == err else float("inf")
        else:
            err, e32 = rel_err(dev[n], r), rel_err(f32[n], r)
        out.append((n, err, e32, bar(n, e32)))
    return out


class ParityLog:
    """The worst err / bar of every (hp, n_hidden, launch, quantity) the tests judged; `judge`
    prints every figure, records it and returns the quantities over their bar."""

    def __init__(self):
        self.worst = {}

    def judge(self, hp, nh, launch, records):
        over = []
        for name, err, e32, b in records:
            ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
            print(f"hp {hp} nh {nh} {launch} {name}: err {err:.2e} e32 {e32:.2e} "
                  f"err/e32 {ratio:.1f} bar {b:.1e}")
            key = (hp, nh, launch, name)
            if key not in self.worst or err / b > self.worst[key][0] / self.worst[key][3]:
                self.worst[key] = (err, e32, ratio, b)
            if not err <= b:
                over.append((launch, name, err, e32, b))
        return over

    def write(self, path):
        with open(path, "w") as f:
            f.write("# worst case per (hp, n_hidden, launch, quantity): device max |err| / scale "
                    "against fp64,\n# e32 (fp32 torch-CPU against fp64), their ratio, the bar "
                    "max(base, 8 * e32)\n")
            f.write(f"{'hp':>3} {'nh':>2} {'launch':<14} {'quantity':<8} {'err':>9} {'e32':>9} "
                    f"{'err/e32':>8} {'bar':>8}\n")
            for (hp, nh, launch, name), (err, e32, ratio, b) in sorted(self.worst.items()):
                f.write(f"{hp:>3} {nh:>2} {launch:<14} {name:<8} {err:>9.2e} {e32:>9.2e} "
                        f"{ratio:>8.1f} {b:>8.1e}\n")


# ---- the cases of the width x depth tests ----
WIDTHS = [24, 64, 90, 128, 150, 192, 200, 256]  # one per NT = hp / 32, half of them padded
SHAPES = [(h, nh) for h in WIDTHS for nh in (1, 2, 3, 4)] + [(40, 8)]
KINDS = {"critic": (4, 1), "actor": (2, 2)}


def pad32(hidden):
    return (hidden + 31) // 32 * 32


def chain_case(d_in, d_out, hidden, nh, M, shift=None):
    """The net and rows of unfused_chain_run, on the CPU: (layers, x, dy). shift = (a, ks, g):
    the same case rescaled by powers of two (shift_layers; x by 2^a, dy by 2^g)."""
    from oracle.td3_oracle import make_mlp_params
    p = make_mlp_params(17, [d_in] + [hidden] * nh + [d_out])
    g = torch.Generator().manual_seed(2000 + M + nh)
    x = (torch.randn(M, d_in, generator=g) * 20).contiguous()
    dy = torch.randn(M, d_out, generator=g) / M
    layers = [(torch.tensor(W), torch.tensor(b)) for W, b in p]
    if shift is not None:
        a, ks, gs = shift
        layers, _ = shift_layers(layers, a, ks)
        x, dy = ldexp32(x, a).contiguous(), ldexp32(dy, gs)
    return layers, x, dy


def chain_quantities(c, nh):
    """mlp_chain's result by quantity name."""
    q = dict(out=c["out"], dx=c["dx"])
    for l in range(nh):
        q[f"h{l}"], q[f"dz{l}"] = c["h"][l], c["dz"][l]
    q.update(ref_grad_tensors(c["grads"]))
    return q


EPOCH_SEEDS = dict(ta=61, tc0=62, tc1=63, cr0=64, cr1=65, actor=66, atgt=67)
RING = 500


def epoch_case(hidden, nh, B, K=None):
    """A TD3 epoch's inputs on the CPU: a ring of 500 random rows (done ~ 10 %), injected sample
    indices of the critic and the actor phase, smoothing noise, and the layers of seven distinct
    nets (target actor, target critics, online critics, actor, the actor's own target).
    K: the joint rescaling of joint_shifts (every critic's layers by shifts of total K, every
    actor's by shifts of total 0, the ring's reward column by 2^K)."""
    from oracle.td3_oracle import make_mlp_params
    g = torch.Generator().manual_seed(9000 + B + nh)
    rows = torch.randn(RING, 8, generator=g) * 10
    rows[:, 7] = (torch.rand(RING, generator=g) < 0.1).float()
    idx = torch.randint(0, RING, (B,), generator=g)
    idx_a = torch.randint(0, RING, (B,), generator=g)
    eps = torch.randn(B, 2, generator=g)
    layers = {}
    for name, seed in EPOCH_SEEDS.items():
        d_in, d_out = (2, 2) if name in ("ta", "actor", "atgt") else (4, 1)
        p = make_mlp_params(seed, [d_in] + [hidden] * nh + [d_out])
        layers[name] = [(torch.tensor(W), torch.tensor(b)) for W, b in p]
    if K is not None:
        ks_actor, ks_critic = joint_shifts(nh, K)
        rows[:, 4] = ldexp32(rows[:, 4], K)
        for name in layers:
            ks = ks_actor if name in ("ta", "actor", "atgt") else ks_critic
            layers[name], _ = shift_layers(layers[name], 0, ks)
    return dict(rows=rows, idx=idx, idx_a=idx_a, eps=eps, layers=layers, B=B, hidden=hidden,
                nh=nh, ring=RING)


def critic_quantities(e, k):
    """critic_epoch's result for online critic k by quantity name."""
    q = dict(dq=e["dq"][k], loss=e["loss"][k].reshape(1))
    q.update(ref_grad_tensors(e["grads"][k]))
    return q


def critic_refs(case, bits, narrow=False):
    """(fp64, fp32[, narrowed]) critic_epoch of an epoch_case, and dq's scale 2 / B * max(max
    |q_i|, max |y|): a bar measured against 2 (q - y) / B itself would vanish where q ~ y."""
    L = case["layers"]
    batch = case["rows"][case["idx"]]
    args = (L["ta"], [L["tc0"], L["tc1"]], [L["cr0"], L["cr1"]], batch, case["eps"], bits)
    ref = critic_epoch(*args)
    out = [ref, critic_epoch(*args, dtype=torch.float32)]
    if narrow:
        out.append(critic_epoch(*args, dtype=torch.float32, narrow=True))
    scale = [2.0 / case["B"] * max(float(ref["q"][k].abs().max()), float(ref["y"].abs().max()))
             for k in range(2)]
    return out, scale


def actor_quantities(e):
    q = dict(q=e["q"], da=e["da"])
    q.update(ref_grad_tensors(e["grads"]))
    return q


def ref_grad_tensors(grads):
    return {n: t for l, (gW, gb) in enumerate(grads) for n, t in ((f"dW{l}", gW), (f"db{l}", gb))}


# ---- the TD3 epochs (robot.py:329-361, 382-390) at a given dtype ----
def f32c(v):
    """The f32 value of a constant the launch takes as a float."""
    return float(torch.tensor(v, dtype=torch.float32))


def critic_epoch(ta, tc, cr, batch, eps, bits, dtype=torch.float64, narrow=False, gamma=0.99,
                 policy_noise=0.2, noise_clip=0.5, max_action=5.0):
    """train_critic (robot.py:329-361) on the sampled f32 rows `batch` [B][8] and the smoothing
    noise eps [B][2]: ta / tc[2] / cr[2] = the layers of the target actor, target critics and
    online critics, bits[i] the online critics' injected ReLU decisions. Returns dict(y [B],
    q[i] [B], dq[i] [B] = 2 (q_i - y) / B, loss[i], zs[i], grads[i])."""
    B = batch.shape[0]
    bt = batch.to(dtype)
    s2, r, nd = bt[:, 5:7], bt[:, 4:5], 1 - bt[:, 7:8]
    noise = (eps.to(dtype) * f32c(policy_noise)).clamp(-f32c(noise_clip), f32c(noise_clip))
    a2 = (mlp_forward(ta, s2, dtype, narrow)[0] + noise).clamp(-f32c(max_action),
                                                                f32c(max_action))
    x2 = torch.cat([s2, a2], 1)
    qt = torch.min(mlp_forward(tc[0], x2, dtype, narrow)[0],
                   mlp_forward(tc[1], x2, dtype, narrow)[0])
    y = r + f32c(gamma) * qt * nd
    out = dict(y=y[:, 0], q=[], dq=[], loss=[], zs=[], grads=[])
    x = bt[:, :4]
    for i in range(2):
        q, zs, hs = mlp_forward(cr[i], x, dtype, narrow)
        dq = 2 * (q - y) / B
        _, _, grads = mlp_backward(cr[i], hs, dq, bits[i], dtype, narrow)
        out["q"].append(q[:, 0])
        out["dq"].append(dq[:, 0])
        out["loss"].append(((q - y) ** 2).mean())
        out["zs"].append(zs)
        out["grads"].append(grads)
    return out


def actor_epoch(actor, critic, batch, bits_a, bits_c, dtype=torch.float64, narrow=False):
    """train_actor (robot.py:382-390), L = -mean Q1(s, pi(s)), on the sampled rows: dict(a, q [B],
    da [B][2] = dL/da, grads (the actor's), zs_a, zs_c, x_c (the critic's input rows))."""
    B = batch.shape[0]
    s = batch[:, :2].to(dtype)
    a, zs_a, hs_a = mlp_forward(actor, s, dtype, narrow)
    x = torch.cat([s, a], 1)
    q, zs_c, hs_c = mlp_forward(critic, x, dtype, narrow)
    dq = torch.full((B, 1), -1.0 / B, dtype=dtype)
    _, dx, _ = mlp_backward(critic, hs_c, dq, bits_c, dtype, narrow)
    da = dx[:, 2:4]
    _, _, grads = mlp_backward(actor, hs_a, da, bits_a, dtype, narrow)
    return dict(a=a, q=q[:, 0], da=da, grads=grads, zs_a=zs_a, zs_c=zs_c, x_c=x)


# ---- the unfused launches: forward -> row backward -> weight gradients -> reduce ----
def unfused_chain_run(d_in, d_out, hidden, nh, M, splits=5, nan_fill=False, shift=None,
                      case=None):
    """nav_mlp_forward -> nav_mlp_backward (every dz row saved) -> nav_mlp_wgrad -> nav_grad_reduce
    of a make_mlp_params(17) net on randn * 20 rows from manual_seed(2000 + M + nh). nan_fill: the
    edge slabs, the weight-gradient slabs and the flat gradient start as NaN. shift = (a, ks, g):
    chain_case's rescaled case; case = (layers, x, dy): those instead. Returns dict(net, layers,
    x, dy, out, acts, dz, dx, grad (CPU tensors), bits, masks)."""
    from nav._lib import descs, lib, parr, ptr, stream_handle
    from nav.mlp import DeviceMLP, forward
    if shift is None and case is None:
        net, layers = make_net(d_in, d_out, hidden, nh, 17)
        _, x, dy = chain_case(d_in, d_out, hidden, nh, M)
    else:
        layers, x, dy = case if case is not None else chain_case(d_in, d_out, hidden, nh, M, shift)
        net = DeviceMLP(d_in, d_out, hidden, nh, DEV).load(
            [(W.numpy(), b.numpy()) for W, b in layers])
    xd, dyd = x.to(DEV), dy.to(DEV)
    out = torch.zeros(M, d_out, device=DEV)
    acts = torch.zeros(nh, M, net.hp, device=DEV)
    masks = net.mask_buffer(M)
    forward([net], xd, d_in, 0, [out], d_out, 0, M, acts=[acts], masks=[masks])
    L = lib()
    s = stream_handle()
    fill = float("nan") if nan_fill else 0.0
    nblk = L.nav_mlp_row_blocks(M)
    eslab = torch.full((nblk, L.nav_mlp_edge_count(d_in, d_out, net.hp, nh)), fill, device=DEV)
    dz = torch.zeros(nh, M, net.hp, device=DEV)
    dx = torch.zeros(M, d_in, device=DEV)
    L.nav_mlp_backward(descs(net), 1, M, parr(dyd), d_out, parr(masks), ptr(xd), d_in, 0,
                       parr(acts[nh - 1]), parr(dz), (1 << nh) - 1, parr(dx), parr(eslab), s)
    hs = torch.full((splits, max(4, L.nav_mlp_hidden_count(net.hp, nh))), fill, device=DEV)
    grad = torch.full((net.count,), fill, device=DEV)
    L.nav_mlp_wgrad(descs(net), 1, M, ptr(xd), d_in, 0, parr(acts), parr(dz), parr(dyd), d_out,
                    parr(masks), parr(hs), splits, s)
    L.nav_grad_reduce(C.byref(net.desc()), ptr(hs), splits, ptr(eslab), nblk, ptr(grad), s)
    torch.cuda.synchronize()
    return dict(net=net, layers=layers, x=x, dy=dy, out=out.cpu(), acts=acts.cpu(), dz=dz.cpu(),
                dx=dx.cpu(), grad=grad.cpu(), bits=relu_bits(masks, nh, net.hp, hidden, M),
                masks=masks.cpu())


def split_gemm_row_errors(d_in, d_out, hidden, nh, M, splits=5, detail=False):
    """The launches and the fp64 reference of test_split_gemm_f32_accuracy_vs_fp64 at M rows.
    Returns (rows, dW): rows[name] = (|err| per row [M] (the row's worst entry), max |ref|) for
    the output, every saved activation h_l, every dz_l and dx; dW[name] = max |err| / max |ref|
    of every hidden x hidden weight gradient. Asserts on the way that the forward's ReLU bits
    equal the fp64 signs outside the rounding band.
    detail: NaN-prefilled gradient buffers, and a third value dict(dev, ref, f32, band, run): the
    device's, the fp64 chain's and the fp32 chain's quantities by name (out, h*, dz*, dx and every
    tensor dW* / db* of the flat gradient), band = relu_band's counts; the device's padded
    columns, rows and slots are checked to be exactly 0."""
    run = unfused_chain_run(d_in, d_out, hidden, nh, M, splits, nan_fill=detail)
    layers, x, dy, bits = run["layers"], run["x"], run["dy"], run["bits"]

    def per_row(a, ref):
        return (a.double() - ref).abs().reshape(M, -1).amax(1), float(ref.abs().max())

    rows, dW = {}, {}
    ref = mlp_chain(layers, x, dy, bits)
    rows["out"] = per_row(run["out"], ref["out"])
    for l in range(nh):
        rows[f"h{l}"] = per_row(run["acts"][l][:, :hidden], ref["h"][l])
    band = relu_band(layers, x, ref["z"], bits)
    for l in range(nh - 1, -1, -1):
        rows[f"dz{l}"] = per_row(run["dz"][l][:, :hidden], ref["dz"][l])
    rows["dx"] = per_row(run["dx"], ref["dx"])
    hp = run["net"].hp
    offs, _ = layer_offsets(d_in, d_out, hp, nh)
    gflat = run["grad"]
    for l in range(1, nh):
        w_off, _, fo, fi = offs[l]
        got = gflat[w_off:w_off + fo * fi].view(fo, fi)[:hidden, :hidden]
        gW = ref["grads"][l][0]
        dW[f"dW{l}"] = float((got.double() - gW).abs().max() / gW.abs().max())
    if not detail:
        return rows, dW
    assert bool((run["acts"][:, :, hidden:] == 0).all())
    assert bool((run["dz"][:, :, hidden:] == 0).all())
    dev = dict(out=run["out"], dx=run["dx"])
    for l in range(nh):
        dev[f"h{l}"], dev[f"dz{l}"] = run["acts"][l][:, :hidden], run["dz"][l][:, :hidden]
    dev.update(flat_grad_tensors(gflat, d_in, d_out, hidden, hp, nh))
    f32 = mlp_chain(layers, x, dy, bits, torch.float32)
    return rows, dW, dict(dev=dev, ref=chain_quantities(ref, nh), f32=chain_quantities(f32, nh),
                          band=band, run=run)


# ---- the fp16 B-operand images ----
def _fp16_image(packed, off, hp):
    """One fp16 B image (split_entry layout [2][hp/16][2][hp][8], then int32 exponents [hp]) as
    its two planes in fp32 [2][K][N] and the per-column exponents."""
    n = hp * hp
    raw = packed[off:off + n].contiguous().view(torch.float16).float()
    P = raw.view(2, hp // 16, 2, hp, 8).permute(0, 1, 2, 4, 3).reshape(2, hp, hp)
    e = packed[off + n:off + n + hp].contiguous().view(torch.int32)
    return P, e


def _pow2_exp(m):
    """mlp_common.h pow2_exp: e with m 2^e in [2^13, 2^14), clamped to +-126; 0 for 0 / inf."""
    import math
    if not (m > 0) or not math.isfinite(m) or m >= 3.0e38:
        return 0
    _, E = math.frexp(m)
    return max(-126, min(126, 14 - E))


def _assert_images_exact(net, tag):
    """Every hidden x hidden weight: the forward image (B[k][n] = W[n][k]) and the backward image
    (B[k][n] = W[k][n]; for d_out = 1 the top layer's is Wt[k][n] = Wo[k] W[k][n] in f32) hold, per column n with e_n = pow2_exp(max_k |B[k][n]|), hi =
    fp16_rne(B 2^e_n) and lo = fp16_rne(B 2^e_n - hi) bit for bit, and (hi + lo) 2^-e_n equals B
    within 2^-22 of the column's max (11 + 11 significant bits)."""
    hp, nh = net.hp, net.n_hidden
    pk = net.packed.detach().cpu()
    flat = net.params.detach().cpu()
    img = hp * hp + hp
    for L in range(1, nh):
        w_off = net.offsets[L][0]
        W = flat[w_off:w_off + hp * hp].view(hp, hp)
        Wb = W
        if net.d_out == 1 and L == nh - 1:  # the top layer's Wt image: Wo[k] * W[k][n] (f32)
            wo = flat[net.offsets[nh][0]:net.offsets[nh][0] + hp]
            Wb = wo[:, None] * W
        for which, off, Bk in (("fwd", (L - 1) * 2 * img, W.t()), ("bwd", (L - 1) * 2 * img + img, Wb)):
            P, e = _fp16_image(pk, off, hp)
            cmax = Bk.abs().max(0).values
            want = torch.tensor([_pow2_exp(float(m)) for m in cmax], dtype=torch.int32)
            assert torch.equal(e, want), (tag, L, which)
            sc = torch.pow(2.0, want.double())
            x = (Bk.double() * sc).float()  # exact: a power of two
            hi = x.half().float()
            assert torch.equal(P[0], hi), (tag, L, which)
            lo = (x - hi).half().float()
            assert torch.equal(P[1], lo), (tag, L, which)
            rec = (P[0].double() + P[1].double()) / sc
            tol = 2.0 ** -22 * cmax.double() + 1e-45
            assert ((rec - Bk.double()).abs() <= tol).all(), (tag, L, which)


# ---- exact rescaling by powers of two ----
# Inputs by 2^a, layer l's weights by 2^k_l and its bias by 2^(a + k_0 + .. + k_l), the incoming
# gradient by 2^g: while nothing leaves the normal f32 range, every f32 chain of the rescaled case
# yields the base case's values times a known power of two, bit for bit (a power of two commutes
# with every rounding). The kernels' scale bookkeeping must do the same.
SHIFT_SETS = {"S1": (7, (20, -35, 15), -9), "S2": (-30, (-12, -11, -10), 25),
              "S3": (40, (10, 10, 10), -60)}
SHIFT_LO, SHIFT_HI, SHIFT_CAP = 2.0 ** -100, 2.0 ** 100, 1e-3


def ldexp32(t, k):
    """t 2^k in f32 (exact while the result is a normal float or 0)."""
    return (t.double() * 2.0 ** k).to(t.dtype)


def layer_ks(ks, nh, fill=3):
    """ks truncated or extended to the nh + 1 layers; a fourth or later layer takes `fill`."""
    ks = tuple(ks)[:nh + 1]
    return ks + (fill,) * (nh + 1 - len(ks))


def shift_set(name, nh):
    """(a, ks, g) of shift set `name` for a net of nh hidden layers."""
    a, ks, g = SHIFT_SETS[name]
    return a, layer_ks(ks, nh), g


def shift_layers(layers, a, ks):
    """(layers', cums): W_l' = W_l 2^k_l, b_l' = b_l 2^cums[l + 1], cums[0] = a, cums[l + 1] =
    cums[l] + k_l (the exponent h_l carries, and the output for l = n_hidden)."""
    assert len(ks) == len(layers)
    cums = [a]
    out = []
    for (W, b), k in zip(layers, ks):
        cums.append(cums[-1] + k)
        out.append((ldexp32(W, k), ldexp32(b, cums[-1])))
    return out, cums


def expected_shifts(a, ks, g):
    """The exponent every quantity of the rescaled chain carries over the base chain's, by
    quantity name: out, h_l, dz_l, dx, dW_l, db_l (l as in chain_quantities)."""
    nh = len(ks) - 1
    cums = [a]
    for k in ks:
        cums.append(cums[-1] + k)
    s = dict(out=cums[nh + 1], dx=g + sum(ks))
    for l in range(nh):
        s[f"h{l}"] = cums[l + 1]
        s[f"dz{l}"] = g + sum(ks[l + 1:])
    for l in range(nh + 1):
        dzl = s[f"dz{l}"] if l < nh else g
        s[f"dW{l}"], s[f"db{l}"] = dzl + cums[l], dzl
    return s


def joint_shifts(nh, K):
    """(ks_actor, ks_critic) of the fused epochs' joint rescaling: the actor's layer shifts (S1's,
    the last one adjusted) sum to 0, so actions keep their magnitude; the critic's are the same
    with K added to the third layer's (or to the last of a shallower net), total K."""
    ks = list(layer_ks(SHIFT_SETS["S1"][1], nh))
    ks[-1] -= sum(ks)
    kc = list(ks)
    kc[min(2, nh)] += K
    return tuple(ks), tuple(kc)


def assert_shifted(got, base, s, name, lo=SHIFT_LO, hi=SHIFT_HI):
    """got == base 2^s bit for bit on every entry whose base value is 0 or whose shifted
    magnitude lies in [lo, hi] = [2^-100, 2^100]; the entries outside that window (where a
    subnormal or an overflow may legitimately round) are left out, and must be at most 1e-3 of
    the non-zero ones. Returns that share."""
    import math
    assert got.shape == base.shape, (name, got.shape, base.shape)
    got, base = got.reshape(-1), base.reshape(-1)
    want = base.double() * 2.0 ** s
    mag = want.abs()
    nz = base != 0
    held = ~nz | ((mag >= lo) & (mag <= hi))
    n_nz = int(nz.sum())
    share = float((~held).sum()) / n_nz if n_nz else 0.0
    assert share <= SHIFT_CAP, f"{name}: {share:.2e} of the non-zero entries leave the window"
    bad = held & ~(got.double() == want)
    n_bad = int(bad.sum())
    if n_bad:
        i = int(bad.nonzero()[0])
        g_, b_ = float(got[i]), float(base[i])
        if b_ != 0 and g_ != 0 and math.isfinite(g_):
            m, e = math.frexp(g_ / b_)
            ratio = f"got / base = {m * 2:.9g} * 2^{e - 1}"
        else:
            ratio = "got / base undefined"
        raise AssertionError(
            f"{name}: {n_bad} of {int(held.sum())} entries differ from base * 2^{s}; first at "
            f"{i}: got {g_!r} base {b_!r} ({ratio}, expected 2^{s})")
    return share


# ---- the cases of the rescaling tests (tests/test_scale_cpu.py, tests/test_gpu_scale.py) ----
SCALE_BIG = 16421  # 64-row blocks: gemm_cols_step and its per-step A scale
# (d_in, d_out, hidden, nh), one per code path: k_wgrad_fact<8> / <4> / <2> with gemm_bits, the
# operand-form k_wgrad, k_wgrad_gen at a padded width, gemm_bits under a padded hp = 96, and a
# net without a hidden x hidden product
SCALE_SHAPES = [(4, 1, 256, 2), (4, 1, 128, 2), (4, 1, 64, 2), (2, 2, 256, 2), (2, 2, 200, 3),
                (4, 1, 90, 3), (4, 1, 24, 1)]
SCALE_CHAIN_CASES = [(s, 97) for s in SCALE_SHAPES] + [((4, 1, 256, 2), SCALE_BIG),
                                                       ((2, 2, 256, 2), SCALE_BIG)]
# the fused epochs: (hidden, nh, B), each at K = -24 and K = +18 (joint_shifts)
SCALE_EPOCH_CASES = [(256, 2, SCALE_BIG), (256, 2, 100), (200, 3, 100), (64, 2, 100)]
SCALE_KS = (-24, 18)
# the ends of the range (held to the fp64 bars, not to bit equality: clamps and caps may bind)
RANGE_SHAPES = [(4, 1, 256, 2), (2, 2, 256, 2), (2, 2, 200, 3)]
RANGE_CASES = [(r, s, 97) for r in ("R1", "R2", "R3", "R4", "R5") for s in RANGE_SHAPES]
RANGE_CASES += [(r, (4, 1, 256, 2), SCALE_BIG) for r in ("R1", "R3")]
ZERO_X_ROWS, ZERO_DY_ROWS, ZERO_W_ROW, ZERO_W_COL = slice(32, 64), slice(64, 96), 5, 9


def range_shift(name, nh):
    """(a, ks, g) of the range ends R1 .. R4: R1 small hidden weights (k_1 = -118, the output
    layer +118: the image's column exponents clamp at 126), R2 large activations (a = +60, k_0 =
    +40, k_1 = -100: h_0 near 2^100), R3 tiny gradients (g = -110), R4 large gradients (g = +70,
    the output layer +20)."""
    ks = [0] * (nh + 1)
    a = g = 0
    if name == "R1":
        ks[1], ks[nh] = ks[1] - 118, ks[nh] + 118
    elif name == "R2":
        a, ks[0], ks[1] = 60, 40, ks[1] - 100
    elif name == "R3":
        g = -110
    elif name == "R4":
        g, ks[nh] = 70, 20
    else:
        raise KeyError(name)
    return a, tuple(ks), g


def range_case(name, d_in, d_out, hidden, nh, M):
    """(layers, x, dy) of a range end: chain_case under range_shift, or R5, the zeros: one whole
    32-row tile of x all zero under zero biases, one row and one column of the first hidden x
    hidden weight all zero (an all-zero column of its forward and of its backward image), dy all
    zero in another 32-row tile."""
    if name != "R5":
        return chain_case(d_in, d_out, hidden, nh, M, range_shift(name, nh))
    layers, x, dy = chain_case(d_in, d_out, hidden, nh, M)
    layers = [(W.clone(), torch.zeros_like(b)) for W, b in layers]
    layers[1][0][ZERO_W_ROW, :] = 0
    layers[1][0][:, ZERO_W_COL] = 0
    x, dy = x.clone(), dy.clone()
    x[ZERO_X_ROWS] = 0
    dy[ZERO_DY_ROWS] = 0
    return layers, x, dy


def forward_signs(layers, x, dtype=torch.float32):
    """The ReLU decisions of a torch-CPU forward at `dtype` (for chains without a device)."""
    return [z > 0 for z in mlp_forward(layers, x, dtype)[1]]
