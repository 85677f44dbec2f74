"""The licence of tests/test_gpu_scale.py, on the CPU: the fp32 torch chain of tests/mlp_ref.py is
exactly equivariant under rescaling by powers of two at every shape and shift set the GPU tests
use (inputs by 2^a, layer l's weights by 2^k_l, its bias by 2^(a + k_0 + .. + k_l), the incoming
gradient by 2^g: every quantity of the rescaled chain is the base chain's times a known power of
two, bit for bit), the entries assert_shifted leaves out stay within its cap, and the fp64 chain
of every rescaled case is finite. The same for the TD3 epochs under the joint shifts, and for the
range ends R1 .. R5, whose chains must stay finite and, as far as their shifts leave the data
itself exact (see EXACT_QUANTITIES), the exact shift of the base."""
import pytest
import torch

import bc_ref as BR
import mlp_ref as R


def _ids(cases):
    return [str(c).replace(" ", "") for c in cases]


def _finite(q):
    return all(bool(torch.isfinite(t).all()) for t in q.values())


def _chain_pair(shape, M, shift, lo=R.SHIFT_LO, hi=R.SHIFT_HI):
    """The fp32 chain of the rescaled case against the base's through assert_shifted; returns the
    rescaled case's fp32 and fp64 quantities and the worst left-out share."""
    d_in, d_out, hidden, nh = shape
    base = R.chain_case(d_in, d_out, hidden, nh, M)
    case = R.chain_case(d_in, d_out, hidden, nh, M, shift)
    bits = R.forward_signs(*base[:2])
    assert all(torch.equal(u, v) for u, v in zip(bits, R.forward_signs(*case[:2])))
    q0 = R.chain_quantities(R.mlp_chain(*base, bits, torch.float32), nh)
    q1 = R.chain_quantities(R.mlp_chain(*case, bits, torch.float32), nh)
    exp = R.expected_shifts(*shift)
    assert exp.keys() == q0.keys()
    share = max(R.assert_shifted(q1[n], q0[n], exp[n], n, lo, hi) for n in q0)
    return q1, R.chain_quantities(R.mlp_chain(*case, bits), nh), share


def test_helpers():
    """shift_layers, expected_shifts, layer_ks and joint_shifts on a hand-checked case; a wrong
    exponent is reported with the ratio's exponent."""
    assert R.layer_ks((20, -35, 15), 1) == (20, -35)
    assert R.layer_ks((20, -35, 15), 4) == (20, -35, 15, 3, 3)
    W, b = torch.tensor([[1.5, -3.0]]), torch.tensor([0.75])
    (W1, b1), (W2, b2) = R.shift_layers([(W, b), (W, b)], 2, (3, -5))[0]
    assert torch.equal(W1, W * 8) and torch.equal(b1, b * 32)
    assert torch.equal(W2, W / 32) and torch.equal(b2, b * 1.0)
    assert R.shift_layers([(W, b), (W, b)], 2, (3, -5))[1] == [2, 5, 0]
    assert R.expected_shifts(7, (20, -35, 15), -9) == dict(
        out=7, dx=-9, h0=27, h1=-8, dz0=-29, dz1=6, dW0=-22, db0=-29, dW1=33, db1=6, dW2=-17,
        db2=-9)
    for nh in (1, 2, 3, 4):
        for K in R.SCALE_KS:
            ka, kc = R.joint_shifts(nh, K)
            assert sum(ka) == 0 and sum(kc) == K and len(ka) == len(kc) == nh + 1
    assert R.joint_shifts(2, -24) == ((20, -35, 15), (20, -35, -9))
    t = torch.tensor([1.0, 0.0, -3.0, 2.0 ** -90])
    assert R.assert_shifted(t * 4, t, 2, "t") == 0.0
    with pytest.raises(AssertionError, match=r"2\^3, expected 2\^2"):
        R.assert_shifted(t * 8, t, 2, "t")
    with pytest.raises(AssertionError, match="entries differ"):
        R.assert_shifted(t * 4 + torch.tensor([0.0, 1e-30, 0.0, 0.0]), t, 2, "t")  # a zero moved
    with pytest.raises(AssertionError, match="leave the window"):
        R.assert_shifted(t / 2.0 ** 20, t, -20, "t")  # 1 of 3 non-zero entries below 2^-100


@pytest.mark.parametrize("name", list(R.SHIFT_SETS))
@pytest.mark.parametrize("shape,M", R.SCALE_CHAIN_CASES, ids=_ids(R.SCALE_CHAIN_CASES))
def test_chain_is_shift_equivariant(shape, M, name):
    f32, f64, share = _chain_pair(shape, M, R.shift_set(name, shape[3]))
    print(f"{shape} M {M} {name}: left-out share {share:.1e}")
    assert _finite(f32) and _finite(f64)


def _epoch_bits(case):
    L = case["layers"]
    batch = case["rows"][case["idx"]]
    rows_a = case["rows"][case["idx_a"]]
    bits = [R.forward_signs(L[f"cr{k}"], batch[:, :4]) for k in range(2)]
    bits_a = R.forward_signs(L["actor"], rows_a[:, :2])
    a = R.mlp_forward(L["actor"], rows_a[:, :2], torch.float32)[0]
    bits_c = R.forward_signs(L["cr0"], torch.cat([rows_a[:, :2], a], 1))
    return batch, rows_a, bits, bits_a, bits_c


def epoch_quantities(case, dtype, bits=None):
    """critic_epoch and actor_epoch of an epoch_case by quantity name (c<k>_*: online critic k;
    a_*: the actor phase), with the ReLU decisions of the case's own fp32 forwards (or `bits`)."""
    L = case["layers"]
    batch, rows_a, b, bits_a, bits_c = bits or _epoch_bits(case)
    e = R.critic_epoch(L["ta"], [L["tc0"], L["tc1"]], [L["cr0"], L["cr1"]], batch, case["eps"], b,
                       dtype=dtype)
    q = {"y": e["y"]}
    for k in range(2):
        q.update({f"c{k}_{n}": t for n, t in R.critic_quantities(e, k).items()})
        q[f"c{k}_q"] = e["q"][k]
    ea = R.actor_epoch(L["actor"], L["cr0"], rows_a, bits_a, bits_c, dtype=dtype)
    q.update({f"a_{n}": t for n, t in R.actor_quantities(ea).items()}, a_a=ea["a"])
    return q


def epoch_shifts(nh, K):
    """The exponent of every quantity of epoch_quantities under the joint shifts of total K."""
    ka, kc = R.joint_shifts(nh, K)
    s = {"y": K, "a_a": 0, "a_q": K, "a_da": K}
    ec, ea = R.expected_shifts(0, kc, K), R.expected_shifts(0, ka, K)
    for n in R.grad_names(nh):
        s["c0_" + n] = s["c1_" + n] = ec[n]
        s["a_" + n] = ea[n]
    for k in range(2):
        s.update({f"c{k}_dq": K, f"c{k}_q": K, f"c{k}_loss": 2 * K})
    return s


@pytest.mark.parametrize("K", R.SCALE_KS)
@pytest.mark.parametrize("hidden,nh,B", R.SCALE_EPOCH_CASES, ids=_ids(R.SCALE_EPOCH_CASES))
def test_epochs_are_shift_equivariant(hidden, nh, B, K):
    base, case = R.epoch_case(hidden, nh, B), R.epoch_case(hidden, nh, B, K)
    assert torch.equal(case["rows"][:, :4], base["rows"][:, :4])
    b0, b1 = _epoch_bits(base), _epoch_bits(case)
    for u, v in zip(b0[2] + [b0[3], b0[4]], b1[2] + [b1[3], b1[4]]):
        assert all(torch.equal(x, y) for x, y in zip(u, v))
    q0, q1 = epoch_quantities(base, torch.float32, b0), epoch_quantities(case, torch.float32, b1)
    exp = epoch_shifts(nh, K)
    assert exp.keys() == q0.keys()
    share = max(R.assert_shifted(q1[n], q0[n], exp[n], n) for n in q0)
    print(f"{hidden} x {nh} B {B} K {K}: left-out share {share:.1e}")
    assert _finite(q1) and _finite(epoch_quantities(case, torch.float64, b1))


@pytest.mark.parametrize("K", R.SCALE_KS)
def test_bc_epoch_is_shift_equivariant(K):
    """actor_epoch_bc at (150, 2), B = 100, 7 demonstration rows, the BC weight times 2^K: q, da
    and the gradients carry their shifts, the BC sum none."""
    hidden, nh, B, bd = 150, 2, 100, 7
    qs = {}
    for k in (None, K):
        c = BR.bc_case(hidden, nh, B, bd, K=k)
        la, lc = c["layers"]["actor"], c["layers"]["cr0"]
        rows = c["rows"][c["idx_a"]]
        bits_a = R.forward_signs(la, rows[:, :2])
        a = R.mlp_forward(la, rows[:, :2], torch.float32)[0]
        bits_c = R.forward_signs(lc, torch.cat([rows[:, :2], a], 1))
        w = 0.5 * 2.0 ** (k or 0)
        qs[k] = [BR.bc_quantities(BR.actor_epoch_bc(la, lc, rows, bits_a, bits_c, bd, 1.0, w,
                                                    dtype=dt))
                 for dt in (torch.float32, torch.float64)]
    ea = R.expected_shifts(0, R.joint_shifts(nh, K)[0], K)
    for n, t in qs[None][0].items():
        s = 0 if n == "loss_bc" else K if n in ("q", "da", "da_demo", "da_rest") else ea[n]
        R.assert_shifted(qs[K][0][n], t, s, n)
    assert _finite(qs[K][0]) and _finite(qs[K][1])


# R1 and R3 cannot be the exact shift of the base throughout: their shifts themselves round data
# into f32's subnormals (R1: the entries of W_1 below 2^-8 of its largest, at 2^-126 and less; R3:
# dy 2^-110, and every dz_l and dx behind it), so the rescaled case is other data. What is upstream
# of the first such rounding is still held to bit equality: h_0 under R1, the whole forward under
# R3. The rest of those two is judged like any other case, against the fp64 chain of the same f32
# data, with e32 measured on that data.
EXACT_QUANTITIES = {"R1": lambda n: n == "h0", "R3": lambda n: n == "out" or n.startswith("h")}


@pytest.mark.parametrize("name,shape,M", R.RANGE_CASES, ids=_ids(R.RANGE_CASES))
def test_range_ends_stay_finite_and_exact(name, shape, M):
    """R1 .. R4: no entry of the fp32 chain is inf or NaN and the fp64 chain is finite; the fp32
    chain is the exact shift of the base on every entry that stays a normal f32 (R2, R4: every
    quantity; R1, R3: the quantities upstream of the shift's own subnormal roundings, see above).
    R5: the zero tiles' rows of every h_l and dz_l are exactly 0."""
    d_in, d_out, hidden, nh = shape
    case = R.range_case(name, d_in, d_out, hidden, nh, M)
    bits = R.forward_signs(*case[:2])
    f32 = R.chain_quantities(R.mlp_chain(*case, bits, torch.float32), nh)
    f64 = R.chain_quantities(R.mlp_chain(*case, bits), nh)
    assert _finite(f32) and _finite(f64)
    for n in f64:
        print(f"{name} {shape} M {M} {n}: e32 {R.rel_err(f32[n], f64[n]):.2e} "
              f"max {float(f64[n].abs().max()):.2e}")
    if name == "R5":
        for l in range(nh):
            assert bool((f32[f"h{l}"][R.ZERO_X_ROWS] == 0).all())
            assert bool((f32[f"dz{l}"][R.ZERO_X_ROWS] == 0).all())
            assert bool((f32[f"dz{l}"][R.ZERO_DY_ROWS] == 0).all())
            assert bool((f32[f"h{l}"][R.ZERO_DY_ROWS] != 0).any())
        return
    base = R.chain_case(d_in, d_out, hidden, nh, M)
    assert all(torch.equal(u, v) for u, v in zip(bits, R.forward_signs(*base[:2])))
    q0 = R.chain_quantities(R.mlp_chain(*base, bits, torch.float32), nh)
    exp = R.expected_shifts(*R.range_shift(name, nh))
    for n in q0:
        if EXACT_QUANTITIES.get(name, lambda n: True)(n):
            R.assert_shifted(f32[n], q0[n], exp[n], n, 2.0 ** -126, 2.0 ** 127)
