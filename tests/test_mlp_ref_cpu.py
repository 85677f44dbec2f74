"""CPU checks of the fp64 reference the width x depth GPU tests judge the kernels by
(tests/mlp_ref.py), on the reference code alone: the hand-written chain and the two TD3 epochs
equal torch autograd in fp64; a deliberately narrowed GEMM (a 16-bit-mantissa evaluation of the
chain substituted for the device's result) is rejected by the bars max(base, 8 * e32) at every
(hidden, n_hidden); and the fp32 evaluation's own ReLU decisions stay within the kink band's cap."""
import pytest
import torch

import mlp_ref as R


def _signs(zs):
    return [z > 0 for z in zs]


@pytest.mark.parametrize("kind", ["critic", "actor"])
@pytest.mark.parametrize("hidden,nh", [(24, 1), (90, 3), (40, 8)])
def test_chain_equals_autograd(kind, hidden, nh):
    d_in, d_out = R.KINDS[kind]
    layers, x, dy = R.chain_case(d_in, d_out, hidden, nh, 33)
    _, zs, _ = R.mlp_forward(layers, x)
    bits = _signs(zs)
    c = R.chain_quantities(R.mlp_chain(layers, x, dy, bits), nh)
    tl = [(W.double().requires_grad_(True), b.double().requires_grad_(True)) for W, b in layers]
    xr = x.double().requires_grad_(True)
    h = xr
    for l, (W, b) in enumerate(tl):
        h = torch.nn.functional.linear(h, W, b)
        if l < nh:
            h = h * bits[l].double()
    (h * dy.double()).sum().backward()
    assert R.rel_err(c["out"], h.detach()) <= 1e-13
    assert R.rel_err(c["dx"], xr.grad) <= 1e-13
    for l, (W, b) in enumerate(tl):
        assert R.rel_err(c[f"dW{l}"], W.grad) <= 1e-13, l
        assert R.rel_err(c[f"db{l}"], b.grad) <= 1e-13, l


@pytest.mark.parametrize("hidden,nh", [(24, 1), (150, 2), (40, 8)])
def test_epochs_equal_autograd(hidden, nh):
    """critic_epoch against autograd of mse_loss(Q_i(s, a), y) and actor_epoch against autograd
    of -mean Q1(s, pi(s)), fp64, ReLU as z * (z > 0)."""
    case = R.epoch_case(hidden, nh, 33)
    L = case["layers"]
    f64 = lambda layers: [(W.double().requires_grad_(True),  # noqa: E731
                           b.double().requires_grad_(True)) for W, b in layers]

    def net(tl, x):
        h = x
        for l, (W, b) in enumerate(tl):
            h = torch.nn.functional.linear(h, W, b)
            if l < nh:
                h = torch.relu(h)
        return h

    batch = case["rows"][case["idx"]]
    bits = [_signs(R.mlp_forward(L[k], batch[:, :4])[1]) for k in ("cr0", "cr1")]
    (ref, _), _ = R.critic_refs(case, bits)
    for k, name in enumerate(("cr0", "cr1")):
        tl = f64(L[name])
        q = net(tl, batch[:, :4].double())
        loss = torch.nn.functional.mse_loss(q[:, 0], ref["y"])
        loss.backward()
        assert abs(loss.item() - float(ref["loss"][k])) <= 1e-13 * loss.item()
        for l, (W, b) in enumerate(tl):
            assert R.rel_err(ref["grads"][k][l][0], W.grad) <= 1e-12, (name, l)
            assert R.rel_err(ref["grads"][k][l][1], b.grad) <= 1e-12, (name, l)
    rows_a = case["rows"][case["idx_a"]]
    s = rows_a[:, :2].double()
    ta = f64(L["actor"])
    a = net(ta, s)
    crit = [(W.double(), b.double()) for W, b in L["cr0"]]
    x = torch.cat([s, a], 1)
    (-net(crit, x).mean()).backward()
    bits_a = _signs(R.mlp_forward(L["actor"], s)[1])
    bits_c = _signs(R.mlp_forward(L["cr0"], x.detach())[1])
    e = R.actor_epoch(L["actor"], L["cr0"], rows_a, bits_a, bits_c)
    for l, (W, b) in enumerate(ta):
        assert R.rel_err(e["grads"][l][0], W.grad) <= 1e-12, l
        assert R.rel_err(e["grads"][l][1], b.grad) <= 1e-12, l


def narrowed_outcome(hidden, nh):
    """The quantities over their bar, per launch family, when the 16-bit-mantissa evaluation of
    the chain stands in for the device: (a) the unfused chain of both network kinds at M = 33 and
    97, (b) the critic epoch and (c) the actor epoch at B = 100. ReLU decisions: the fp64 signs."""
    log = R.ParityLog()
    hp = R.pad32(hidden)
    over = dict(a=[], b=[], c=[])
    for kind, (d_in, d_out) in R.KINDS.items():
        for M in (33, 97):
            layers, x, dy = R.chain_case(d_in, d_out, hidden, nh, M)
            bits = _signs(R.mlp_forward(layers, x)[1])
            ev = [R.chain_quantities(R.mlp_chain(layers, x, dy, bits, dt, nw), nh)
                  for dt, nw in ((torch.float64, False), (torch.float32, False),
                                 (torch.float32, True))]
            over["a"] += log.judge(hp, nh, f"chain_{kind}", R.compare(ev[2], ev[0], ev[1]))
    case = R.epoch_case(hidden, nh, 100)
    L = case["layers"]
    batch = case["rows"][case["idx"]]
    bits = [_signs(R.mlp_forward(L[k], batch[:, :4])[1]) for k in ("cr0", "cr1")]
    (ref, f32, nar), scale = R.critic_refs(case, bits, narrow=True)
    for k in range(2):
        over["b"] += log.judge(hp, nh, "critic_rows", R.compare(
            R.critic_quantities(nar, k), R.critic_quantities(ref, k), R.critic_quantities(f32, k),
            scales={"dq": scale[k]}))
    rows_a = case["rows"][case["idx_a"]]
    s = rows_a[:, :2]
    a64, zs_a, _ = R.mlp_forward(L["actor"], s)
    bits_a = _signs(zs_a)
    bits_c = _signs(R.mlp_forward(L["cr0"], torch.cat([s.double(), a64], 1))[1])
    ev = [R.actor_quantities(R.actor_epoch(L["actor"], L["cr0"], rows_a, bits_a, bits_c, dt, nw))
          for dt, nw in ((torch.float64, False), (torch.float32, False), (torch.float32, True))]
    over["c"] += log.judge(hp, nh, "actor_rows", R.compare(ev[2], ev[0], ev[1]))
    return over


@pytest.mark.parametrize("hidden,nh", R.SHAPES)
def test_narrowed_gemm_is_rejected(hidden, nh):
    over = narrowed_outcome(hidden, nh)
    for fam in "abc":
        assert over[fam], (hidden, nh, fam)


def test_reference_stays_within_the_band_cap():
    """The fp32 evaluation's ReLU decisions against the fp64 signs, over every shape and row
    count of the width x depth tests' unfused chain: equal outside the band, and inside it at
    most max(2, 5e-4 * entries) entries per case."""
    worst = 0.0
    for hidden, nh in R.SHAPES:
        for d_in, d_out in R.KINDS.values():
            for M in (1, 33, 97):
                layers, x, _ = R.chain_case(d_in, d_out, hidden, nh, M)
                _, zs, _ = R.mlp_forward(layers, x)
                bits = _signs(R.mlp_forward(layers, x, torch.float32)[1])
                inside, entries = R.relu_band(layers, x, zs, bits)
                R.assert_band_cap(inside, entries)
                worst = max(worst, inside / entries)
    print(f"worst share inside the band: {worst:.2e}")
