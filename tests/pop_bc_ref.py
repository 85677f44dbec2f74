"""What the CPU and GPU tests of the population's demonstration learning share: the shape of the
kernel cases' rings, the members' seeds, the host restatement of nav_td3_mix_idx and the member
that is also judged against fp64 (tests/bc_ref.py's case at hidden 64 x 2, B = 100, B_demo = 7, on
the indices the mix draws for it). Imports no GPU code."""
import torch

import bc_ref as BR
import mlp_ref as R

CAP, FILL, N_TAIL, COUNTER = 512, 300, BR.N_DEMO, 3
FP64 = dict(hidden=64, nh=2, B=100, b_demo=7, member=1)


def member_seed(m):
    return 1000 + 17 * m


def host_mix_idx(orc, seed, B, b_demo, size, demo_base, n_demo, counter, actor):
    """nav_td3_mix_idx's array on the host: the oracle's Philox at ctr = (b, 0, tag, 2 * counter
    [+ 1 for the actor's]), tag NAV_TAG_DEMO = 7 over the tail for rows < b_demo, NAV_TAG_SAMPLE =
    4 over the ring's fill for the rest."""
    key = (seed & 0xFFFFFFFF, seed >> 32)
    out = []
    for b in range(B):
        demo = b < b_demo
        w = orc.philox((b, 0, 7 if demo else 4, 2 * counter + int(actor)), key)[0]
        out.append(demo_base + ((w * n_demo) >> 32) if demo else (w * size) >> 32)
    return out


def fp64_member_rows():
    """(bc_case, storage [CAP + N_TAIL][8]): the case's ring of R.RING rows at the head of a ring
    of CAP (the rows between are never sampled: FILL < R.RING), its tail behind it."""
    case = BR.bc_case(FP64["hidden"], FP64["nh"], FP64["B"], FP64["b_demo"])
    rows = torch.zeros(CAP + N_TAIL, 8)
    rows[:R.RING] = case["rows"][:R.RING]
    rows[CAP:] = case["rows"][R.RING:]
    return case, rows
