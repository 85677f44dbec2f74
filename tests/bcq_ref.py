"""The torch restatement of the Q-filtered behaviour-cloning form of the actor row kernel
(nav_td3_actor_rows_bcq), built from oracle/td3_oracle.py's MLP with autograd, and the cases the
CPU and GPU tests share:

  L = -q_weight * mean_{b<B} Q1(s_b, pi(s_b))
      + bc_weight * (1/B_demo) * sum_{b<B_demo, keep_b} sum_j (pi_j(s_b) - a_{b,j})^2
  keep_b = Q1(s_b, a_b) > Q1(s_b, pi(s_b))    (strict; no gradient through the decision)

a_b = the sampled row's own action columns; the normaliser stays B_demo whatever the filter keeps.
Imports no GPU code: test_bcq_cpu.py runs it on the CPU."""
import torch

from oracle.td3_oracle import MLP, make_mlp_params

import mlp_ref as R

N_ROWS = 600  # the rows the cases sample from
# the filter's band: a demonstration row whose fp64 margin |Q1(s, a) - Q1(s, pi(s))| is below
# BAND * max |q| is undecided (either answer of the kernel is right there)
BAND = 1e-5
# (hidden, n_hidden, B, B_demo): a block straddling the prefix end; one hidden layer, every row a
# demonstration; saved middle layers and a ragged last block; hp = 256 with the prefix ending on a
# block edge; a single demonstration row; 64-row blocks (B > 16384), one of them straddling
CASES = [(64, 2, 200, 50), (64, 1, 200, 200), (96, 3, 1031, 257), (256, 2, 200, 64),
         (256, 2, 1031, 1), (256, 2, 16421, 4100)]
# the seed of each case's networks and rows, chosen with the fp64 restatement alone
# (test_bcq_cpu.py::test_cases_meet_the_input_conditions)
SEEDS = dict(zip(CASES, (1, 1, 2, 2, 4, 2)))


def _net(layers, dtype, grad):
    m = MLP.__new__(MLP)
    m.params = [(W.to(dtype).clone().requires_grad_(grad), b.to(dtype).clone().requires_grad_(grad))
                for W, b in layers]
    return m


def bcq_epoch(actor, critic, batch, b_demo, q_weight, bc_weight, keep=None, bits_a=None,
              bits_c=None, dtype=torch.float64):
    """One actor epoch of the loss above on the sampled f32 rows `batch` [B][8]. actor / critic:
    [(W, b)] f32 layers. keep: bool [b_demo], the filter's decisions to use (None: formed here as
    q_demo > q). bits_a / bits_c: injected ReLU decisions of the actor's forward and the critic's
    (s, pi(s)) forward (MLP.forward's). The two coefficients enter as the f32 values the launch
    takes, f32(-q_weight / B) and f32(2 * bc_weight / B_demo). Returns dict(a, q [B], q_demo
    [b_demo], keep, da [B][2] = dL/da, bc [1] = the sum over kept rows and components of (pi_j -
    a_j)^2, grads / grads_c = [(dL/dW_l, dL/db_l)] of the actor / critic by autograd)."""
    B = batch.shape[0]
    A, Cn = _net(actor, dtype, True), _net(critic, dtype, True)
    s, a_demo = batch[:, :2].to(dtype), batch[:, 2:4].to(dtype)
    pi = A.forward(s, bits_a)
    pi.retain_grad()
    q = Cn.forward(torch.cat([s, pi], 1), bits_c)[:, 0]
    with torch.no_grad():
        q_demo = Cn.forward(torch.cat([s, a_demo], 1))[:b_demo, 0]
        if keep is None:
            keep = q_demo > q[:b_demo]
    keep = keep.bool()
    d = pi[:b_demo] - a_demo[:b_demo]
    bc = ((d * d).sum(1) * keep.to(dtype)).sum()
    loss = R.f32c(-q_weight / B) * q.sum()
    if b_demo:
        loss = loss + 0.5 * R.f32c(2.0 * bc_weight / b_demo) * bc
    loss.backward()
    z = torch.zeros_like
    grads = [(W.grad if W.grad is not None else z(W), b.grad if b.grad is not None else z(b))
             for W, b in A.params]
    grads_c = [(W.grad if W.grad is not None else z(W), b.grad if b.grad is not None else z(b))
               for W, b in Cn.params]
    return dict(a=pi.detach(), q=q.detach(), q_demo=q_demo, keep=keep, da=pi.grad,
                bc=bc.detach().reshape(1), grads=grads, grads_c=grads_c, n_demo_rows=b_demo)


def bcq_case(hidden, nh, B, b_demo, seed=None):
    """Default-initialised actor and critic (make_mlp_params: the Kaiming-uniform bound) of the
    shape, N_ROWS rows with states uniform in [0, 100]^2 and actions uniform in +-5, and B sample
    indices into them."""
    seed = SEEDS[(hidden, nh, B, b_demo)] if seed is None else seed
    g = torch.Generator().manual_seed(40000 + 1000 * seed + nh)
    rows = torch.randn(N_ROWS, 8, generator=g) * 10
    rows[:, 0:2] = torch.rand(N_ROWS, 2, generator=g) * 100
    rows[:, 2:4] = torch.rand(N_ROWS, 2, generator=g) * 10 - 5
    rows[:, 7] = 0.0
    idx = torch.randint(0, N_ROWS, (B,), generator=g)
    layers = {}
    for k, (name, d_in, d_out) in enumerate((("actor", 2, 2), ("cr0", 4, 1))):
        p = make_mlp_params(100 * seed + k, [d_in] + [hidden] * nh + [d_out])
        layers[name] = [(torch.tensor(W), torch.tensor(b)) for W, b in p]
    return dict(rows=rows.contiguous(), idx_a=idx, layers=layers, B=B, b_demo=b_demo,
                hidden=hidden, nh=nh, ring=N_ROWS)


def filter_shares(ref):
    """(kept, dropped, undecided) shares of the demonstration rows of bcq_epoch's fp64 result,
    and the undecided rows' mask: margin below BAND * max |q|."""
    n = ref["q_demo"].numel()
    margin = (ref["q_demo"] - ref["q"][:n]).abs()
    undecided = margin < BAND * float(ref["q"].abs().max())
    kept = ref["keep"] & ~undecided
    dropped = ~ref["keep"] & ~undecided
    return (float(kept.sum()) / n, float(dropped.sum()) / n, float(undecided.sum()) / n,
            undecided)


def bcq_quantities(e):
    """bcq_epoch's result by quantity name, as bc_ref.bc_quantities names them (the BC sum
    `loss_bc`: mlp_ref.bar holds it to the bar of a cross-row sum)."""
    q = dict(da=e["da"], loss_bc=e["bc"], q=e["q"])
    n = e["n_demo_rows"]
    if 0 < n < e["da"].shape[0]:
        q.update(da_demo=e["da"][:n], da_rest=e["da"][n:])
    q.update(R.ref_grad_tensors(e["grads"]))
    return q
