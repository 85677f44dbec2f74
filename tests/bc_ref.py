"""The fp64 reference of the actor row kernel's behaviour-cloning forms (nav_td3_actor_rows_bc)
and the cases the CPU and GPU tests share: mlp_ref.actor_epoch extended with the BC term

  L = -q_weight * mean_{b<B} Q1(s_b, pi(s_b))
      + bc_weight * (1/B_demo) * sum_{b<B_demo} sum_j (pi_j(s_b) - a_{b,j})^2

(a_b = the sampled row's own action columns; critic None = the BC term alone). Imports no GPU
code: test_bc_cpu.py runs the chains on the CPU."""
import torch

import mlp_ref as R

N_DEMO = 37   # demonstration rows behind epoch_case's ring of R.RING rows


def bc_case(hidden, nh, B, b_demo, K=None):
    """mlp_ref.epoch_case with a demonstration tail: N_DEMO more rows of the ring's own kind
    (random rows, done = 0) behind it, and actor sample indices whose first b_demo entries
    address the tail. K: epoch_case's joint rescaling (the tail's reward column by 2^K as well)."""
    case = R.epoch_case(hidden, nh, B, K)
    g = torch.Generator().manual_seed(7000 + B + nh + b_demo)
    tail = torch.randn(N_DEMO, 8, generator=g) * 10
    tail[:, 7] = 0.0
    if K is not None:
        tail[:, 4] = R.ldexp32(tail[:, 4], K)
    rows = torch.cat([case["rows"], tail], 0).contiguous()
    idx_a = case["idx_a"].clone()
    idx_a[:b_demo] = R.RING + torch.randint(0, N_DEMO, (b_demo,), generator=g)
    case.update(rows=rows, idx_a=idx_a, b_demo=b_demo)
    return case


def actor_epoch_bc(actor, critic, batch, bits_a, bits_c, b_demo, q_weight, bc_weight,
                   dtype=torch.float64, narrow=False):
    """mlp_ref.actor_epoch with the BC term on the batch's first b_demo rows; critic None: the BC
    term alone (q absent). The two coefficients enter as the f32 values the launch takes:
    f32(-q_weight / B) and f32(2 * bc_weight / b_demo). Returns actor_epoch's dict plus bc (the
    sum over demonstration rows and components of (pi_j - a_j)^2, [1])."""
    B = batch.shape[0]
    s = batch[:, :2].to(dtype)
    a, zs_a, hs_a = R.mlp_forward(actor, s, dtype, narrow)
    out = dict(a=a, zs_a=zs_a)
    da = torch.zeros(B, 2, dtype=dtype)
    if critic is not None:
        x = torch.cat([s, a], 1)
        q, zs_c, hs_c = R.mlp_forward(critic, x, dtype, narrow)
        dq = torch.full((B, 1), R.f32c(-q_weight / B), dtype=dtype)
        _, dx, _ = R.mlp_backward(critic, hs_c, dq, bits_c, dtype, narrow)
        da = dx[:, 2:4].clone()
        out.update(q=q[:, 0], zs_c=zs_c, x_c=x)
    d = a[:b_demo] - batch[:b_demo, 2:4].to(dtype)
    if b_demo:
        da[:b_demo] += R.f32c(2.0 * bc_weight / b_demo) * d
    _, _, grads = R.mlp_backward(actor, hs_a, da, bits_a, dtype, narrow)
    out.update(da=da, grads=grads, bc=(d * d).sum().reshape(1), n_demo_rows=b_demo)
    return out


def bc_quantities(e):
    """actor_epoch_bc's result by quantity name; the BC sum is named `loss_bc`, so mlp_ref.bar
    holds it to the bar of a cross-row sum."""
    q = dict(da=e["da"], loss_bc=e["bc"])
    n = e["n_demo_rows"]
    if 0 < n < e["da"].shape[0]:  # each kind of row against its own scale as well
        q.update(da_demo=e["da"][:n], da_rest=e["da"][n:])
    if "q" in e:
        q["q"] = e["q"]
    q.update(R.ref_grad_tensors(e["grads"]))
    return q


def forward_bits(layers, x):
    """The fp64 forward's own ReLU decisions of every hidden layer (for CPU-only chains)."""
    _, zs, _ = R.mlp_forward(layers, x)
    return [z > 0 for z in zs]
