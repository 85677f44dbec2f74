"""td3_update under an active timer (nav.prof) against the plain run: TD3 issues every launch in one
place (TD3._run), inside prof.region only while a timer is active, so a timed update must leave
the very bits of an untimed one, and the timer must see the launches under the names and work
counts bench.py --full reads. Smallest shapes at which the paths can part: 32 x 3 (k_wgrad with a
saved middle layer) and 64 x 2 (k_wgrad_fact for the critics), batch 100 (a partial 32-row block).
The same for the two other modes of the epoch loop: learning from demonstrations (a 64-row tail,
25 demonstration rows per batch: no multiple of 32) and prioritised replay (a stamped ring).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, RING, EPOCHS = 100, 512, 4
SHAPES = [(32, 3), (64, 2)]
TAIL, DEMO_FRACTION, BC_WEIGHT = 64, 0.25, 0.5  # b_demo = 25
PER_ALPHA = 0.6


class _NoHook:
    """A grad_hook of a world of one: the bucket stays as the reduce wrote it."""
    world_size = 1

    def __call__(self, bucket):
        pass


@functools.lru_cache(maxsize=None)
def _update(hidden, nh, timer, hook, mode=None):
    """4 epochs of td3_update from the seed's initial networks on the seeded ring; timer: None,
    "all" (KernelTimer()) or "none" (KernelTimer([]), the plain bench's); mode: None, "demo"
    (demo_fraction 0.25, bc_weight 0.5, a seeded tail of 64 rows) or "per" (per_alpha 0.6, every
    row stamped). -> (state, summary, td3)"""
    from nav import _lib, prof
    from nav import config as K
    from nav.td3 import TD3
    from nav.vec_env import ReplayRing
    _lib.require_gpu()
    extra = {"demo": dict(demo_fraction=DEMO_FRACTION, bc_weight=BC_WEIGHT),
             "per": dict(per_alpha=PER_ALPHA)}.get(mode, {})
    cfg = K.TD3Config(batch_size=B, num_epochs=EPOCHS, policy_update_delay=2,
                      net=K.NetConfig(hidden=hidden, n_hidden=nh), **extra)
    td3 = TD3(cfg, DEV, seed=4321, grad_hook=_NoHook() if hook else None)
    rng = np.random.default_rng(9)
    ring = ReplayRing(RING, DEV, tail=TAIL if mode == "demo" else 0, priorities=mode == "per")
    ring.rows.copy_(torch.tensor(rng.uniform(-5, 5, (RING, 8)).astype(np.float32)))
    ring.rows[:, 7] = (ring.rows[:, 7] > 4.8).float()  # ~2 % dones
    ring.size = RING
    if mode == "demo":
        assert td3.b_demo() == 25
        ring.tail.copy_(torch.tensor(rng.uniform(-5, 5, (TAIL, 8)).astype(np.float32)))
        ring.tail[:, 7] = 0
    if mode == "per":
        ring.stamp(0, RING)
    summary = None
    if timer is None:
        td3.td3_update(ring)
    else:
        t = prof.KernelTimer() if timer == "all" else prof.KernelTimer([])
        with prof.timing(t):
            td3.td3_update(ring)
        summary = t.summary()
    torch.cuda.synchronize()
    state = {"update_counter": td3.update_counter, "mix_launches": td3.mix_launches,
             "per_launches": td3.per_launches}
    if mode == "demo":
        state["bc_part"] = td3.bc_part.clone()
    if mode == "per":
        state["pri"], state["stat"] = ring.pri.clone(), ring.stat.clone()
    for name, net in td3.networks().items():
        state[name + ".params"] = net.params.clone()
        state[name + ".packed"] = net.packed.clone()
    for name, o in (("actor", td3.actor_optimizer), ("critic1", td3.critic_optimizer_1),
                    ("critic2", td3.critic_optimizer_2)):
        state[name + ".m"], state[name + ".v"] = o.m.clone(), o.v.clone()
        state[name + ".t"] = o.step_count
    return state, summary, td3


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k, v in a.items():
        if torch.is_tensor(v):
            assert torch.equal(v, b[k]), k
        else:
            assert v == b[k], k


def _expected(td3, hidden, nh, hook, mode=None):
    """The regions of 4 epochs (policy epochs 0 and 2) with their launch counts and total work:
    the formulas written out."""
    from nav._lib import lib
    L = lib()
    h, hp = hidden, td3.actor_network.hp
    fwd = lambda di, do: 2.0 * B * (di * h + (nh - 1) * h * h + h * do)  # noqa: E731

    def bwd(di, do, dx=False, edges=False, wo=False):
        f = do * h + (nh - 1) * h * h + (h * di if dx else 0)
        if edges:
            f += di * h + 0.5 * nh * h + (do * h if wo else 0)
        return 2.0 * B * f
    wg = 2.0 * B * (nh - 1) * h * h  # one net's hidden x hidden weight gradients
    nblk = L.nav_mlp_row_blocks(B)
    assert nblk == 4  # 100 rows: three whole 32-row blocks and a partial one

    def red_bytes(n, d_in, d_out, count):
        splits = L.nav_mlp_wgrad_splits(n, d_out, hp, nh, B)
        ec = L.nav_mlp_edge_count(d_in, d_out, hp, nh)
        return n * 4.0 * (splits * (count - ec) + nblk * ec + (1 if hook else 4) * count)
    ca, cc = td3.actor_network.count, td3.critic_network_1.count
    exp = {
        "critic_rows": (4, 4 * (fwd(2, 2) + 4 * fwd(4, 1) + 2 * bwd(4, 1, False, True))),
        "actor_rows": (2, 2 * (fwd(2, 2) + fwd(4, 1) + bwd(4, 1, True) +
                               bwd(2, 2, False, True, True))),
        "grad_reduce": (6, 4 * red_bytes(2, 4, 1, cc) + 2 * red_bytes(1, 2, 2, ca)),
    }
    # 6 weight-gradient launches: the twin critics' (work 2 wg) x 4, the actor's x 2. The critics
    # of a 2-hidden-layer net with whole 64-wide tiles run k_wgrad_fact, timed under its own name
    if nh == 2 and hp % 64 == 0:
        exp["mlp_wgrad_fact"] = (4, 4 * 2 * wg)
        exp["mlp_wgrad"] = (2, 2 * wg)
    else:
        exp["mlp_wgrad"] = (6, 4 * 2 * wg + 2 * wg)
    if hook:  # one message per bucket: [critic 1 | critic 2] x 4, the actor's x 2
        exp["allreduce"] = (6, 4 * (2 * cc * 4.0) + 2 * (ca * 4.0))
    if mode == "demo":  # one mix per epoch (both batches' indices), the BC form of the actor rows
        exp["mix_idx"] = (4, 4 * 16.0 * B)
        exp["actor_rows_bc"] = exp.pop("actor_rows")
    if mode == "per":  # the sum hierarchy, one sample and one priority update per epoch, around
        # the weighted form of the critic rows
        exp["per_sums"] = (4, 4 * 4.0 * RING)
        exp["per_sample"] = (4, 4 * 16.0 * B)
        exp["critic_rows_w"] = exp.pop("critic_rows")
        exp["per_update"] = (4, 4 * 20.0 * B)
    return exp


def _assert_summary(summary, exp):
    got = {k: (v["launches"], v["work"]) for k, v in summary.items()}
    print(got)
    assert got == exp
    for k, (n, work) in exp.items():
        assert summary[k]["work_per_launch"] == work / n, k


@pytest.mark.parametrize("hidden,nh", SHAPES)
def test_timed_update_bit_equal_and_regions(hidden, nh):
    ref, _, _ = _update(hidden, nh, None, False)
    assert ref["update_counter"] == EPOCHS and ref["actor.t"] == 2 and ref["critic1.t"] == 4
    full, summary, td3 = _update(hidden, nh, "all", False)
    _assert_same(ref, full)
    _assert_summary(summary, _expected(td3, hidden, nh, False))
    empty, nothing, _ = _update(hidden, nh, "none", False)
    _assert_same(ref, empty)
    assert nothing == {}


@pytest.mark.parametrize("hidden,nh", SHAPES)
def test_timed_update_with_hook_bit_equal_and_regions(hidden, nh):
    ref, _, _ = _update(hidden, nh, None, True)
    full, summary, td3 = _update(hidden, nh, "all", True)
    _assert_same(ref, full)
    _assert_summary(summary, _expected(td3, hidden, nh, True))


@pytest.mark.parametrize("hidden,nh", SHAPES)
def test_timed_demo_update_bit_equal_and_regions(hidden, nh):
    ref, _, _ = _update(hidden, nh, None, False, "demo")
    assert ref["update_counter"] == EPOCHS and ref["actor.t"] == 2 and ref["critic1.t"] == 4
    assert ref["mix_launches"] == 4 and ref["per_launches"] == 0
    assert ref["bc_part"].sum().item() > 0
    full, summary, td3 = _update(hidden, nh, "all", False, "demo")
    _assert_same(ref, full)
    _assert_summary(summary, _expected(td3, hidden, nh, False, "demo"))


@pytest.mark.parametrize("hidden,nh", SHAPES)
def test_timed_per_update_bit_equal_and_regions(hidden, nh):
    ref, _, _ = _update(hidden, nh, None, False, "per")
    assert ref["update_counter"] == EPOCHS and ref["actor.t"] == 2 and ref["critic1.t"] == 4
    assert ref["per_launches"] == 12 and ref["mix_launches"] == 0
    full, summary, td3 = _update(hidden, nh, "all", False, "per")
    _assert_same(ref, full)
    _assert_summary(summary, _expected(td3, hidden, nh, False, "per"))
