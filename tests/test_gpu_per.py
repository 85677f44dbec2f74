"""Prioritised replay on the GPU: the priority store's kernels (nav_per_*) against the host
restatement tests/per_ref.py element for element, the weighted critic row kernel
(nav_td3_critic_rows_w) against the plain launch bit for bit where they must agree and against
fp64 where they differ, and the trainer's plumbing (off means off, the first epoch is a plain
one, later epochs follow the restatement, checkpoints, the rejected combinations).

Integer results are exact. The two double pow()s may differ in their last bit between the device
and numpy, which can move an f32 weight by one ulp and a stored priority by one count: those are
the only slacks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import launches as LN
import mlp_ref as R
import per_ref as P
from gpu_support import nav, ulps_f32  # noqa: F401
from pop_support import params as _params, same as _same, snapshot

pytestmark = pytest.mark.gpu
DEV = R.DEV
SEED, SLO, SHI = LN.SEED, LN.SLO, LN.SHI
MAXP = P.MAX_PRI


# ---------------------------------------------------------------- the priority store
class Store:
    """pri / sums / stat on the device and their nav_per descriptor."""

    def __init__(self, capacity, pri=None):
        from nav._lib import NavPer, lib
        self.L = lib()
        self.capacity = capacity
        host = np.zeros(capacity, np.uint32) if pri is None else np.asarray(pri, np.uint32)
        assert host.shape == (capacity,)
        self.pri = torch.from_numpy(host.view(np.int32).copy()).to(DEV)
        self.sums = torch.zeros(self.L.nav_per_sums_count(capacity), dtype=torch.int64, device=DEV)
        self.stat = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.desc = NavPer(self.pri.data_ptr(), self.sums.data_ptr(), self.stat.data_ptr(),
                           capacity)
        self.ref = C.byref(self.desc)

    def pri_host(self):
        return self.pri.cpu().numpy().view(np.uint32).astype(np.int64)

    def stat_host(self):
        return self.stat.cpu().numpy().view(np.uint32).astype(np.int64)

    def sample(self, size, B, counter, beta, critic=True, weights=True, actor=True):
        from nav._lib import ptr, stream_handle
        ic = torch.full((B,), -1, dtype=torch.int64, device=DEV) if critic else None
        ia = torch.full((B,), -1, dtype=torch.int64, device=DEV) if actor else None
        w = torch.full((B,), float("nan"), device=DEV) if weights else None
        self.L.nav_per_sample(self.ref, size, B, SLO, SHI, counter, beta, ptr(ic), ptr(w), ptr(ia),
                              stream_handle())
        torch.cuda.synchronize()
        return tuple(None if t is None else t.cpu().numpy() for t in (ic, w, ia))


def ulps(a, b):
    """|a - b| in f32 steps, for non-negative finite floats"""
    return ulps_f32(a, b, nonneg=True)


RINGS = [(3000, 2500), (3000, 1), (4096, 4096), ((1 << 20) + 37, (1 << 20) + 5)]
SETS = ["random", "equal", "one_large", "last_row"]


def priority_set(kind, capacity, size):
    rng = np.random.default_rng(capacity + size)
    pri = np.empty(capacity, np.int64)
    if kind == "random":
        pri[:size] = rng.integers(1, MAXP + 1, size)
    elif kind == "equal":
        pri[:size] = 48211
    elif kind == "one_large":
        pri[:size] = 1
        pri[int(rng.integers(0, size))] = MAXP
    else:  # all mass in row size - 1
        pri[:size] = 0
        pri[size - 1] = 77777
    pri[size:] = 0xFFFFFFFF  # rows at or beyond size: never read as priorities
    return pri


@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("capacity,size", RINGS, ids=[f"{c}-{s}" for c, s in RINGS])
def test_sums_and_sample_follow_the_restatement(nav, capacity, size, kind):
    from nav._lib import stream_handle
    pri = priority_set(kind, capacity, size)
    st = Store(capacity, pri)
    st.L.nav_per_sums(st.ref, size, stream_handle())
    beta, counter = 0.4, 9
    prefix = P.prefix(pri, size)
    for B in (100, 257):
        ic, w, ia = st.sample(size, B, counter, beta)
        assert st.stat_host()[1] == int(pri[:size].min())
        for got, actor in ((ic, False), (ia, True)):
            want = P.sample(pri, size, B, SEED, counter, actor, prefix)
            assert np.array_equal(got, want), (B, actor)
        want_w = P.weights(pri, size, ic, beta)
        d = ulps(w, want_w)
        print(f"{kind} {capacity}/{size} B {B}: weight ulps max {d.max()}")
        assert d.max() <= 1
        if kind == "equal":
            assert (w == np.float32(1.0)).all()
        assert (w <= 1).all()
    # the priorities and the rows beyond size are left as they were
    assert np.array_equal(st.pri_host(), pri)


def test_sample_outputs_are_optional(nav):
    from nav._lib import stream_handle
    pri = priority_set("random", 3000, 2500)
    st = Store(3000, pri)
    st.L.nav_per_sums(st.ref, 2500, stream_handle())
    ic, w, ia = st.sample(2500, 257, 4, 0.7)
    ic2, w2, ia2 = st.sample(2500, 257, 4, 0.7, actor=False)
    assert ia2 is None and np.array_equal(ic, ic2) and np.array_equal(w, w2)
    ic3, w3, ia3 = st.sample(2500, 257, 4, 0.7, critic=False, weights=False)
    assert ic3 is None and w3 is None and np.array_equal(ia, ia3)
    ic4, w4, _ = st.sample(2500, 257, 4, 0.7, weights=False)
    assert w4 is None and np.array_equal(ic, ic4)
    # beta = 0: every weight 1
    assert (st.sample(2500, 257, 4, 0.0)[1] == np.float32(1.0)).all()
    # another counter: other draws; the actor's stream of counter c is not the critic's of c
    assert not np.array_equal(ic, st.sample(2500, 257, 5, 0.7)[0])
    assert not np.array_equal(ic, ia)


def test_boundary_targets(nav):
    """A ring of 70 rows with known prefix sums; draws whose target t is P_k - 1 (the last unit of
    row k) and P_k (the first of the next row with mass) are found by host search over the Philox
    stream, then the device must place them as the restatement does."""
    from nav._lib import stream_handle
    size = capacity = 70
    rng = np.random.default_rng(70)
    pri = rng.integers(200, 2000, size).astype(np.int64)
    pri[[7, 8, 40]] = 0  # rows without mass right after a boundary
    prefix = P.prefix(pri, size)
    S, edges = prefix[-1], set(prefix[:-1])
    B, found = 257, {"last": [], "first": []}
    for counter in range(400):
        for actor in (False, True):
            t = P.targets(S, B, SEED, counter, actor)
            for b, v in enumerate(t):
                if v + 1 in edges or v + 1 == S:
                    found["last"].append((counter, actor, b))
                if v in edges:
                    found["first"].append((counter, actor, b))
        if found["last"] and found["first"]:
            break
    assert found["last"] and found["first"], found
    st = Store(capacity, pri)
    st.L.nav_per_sums(st.ref, size, stream_handle())
    for kind, hits in found.items():
        for counter, actor, b in hits:
            ic, _, ia = st.sample(size, B, counter, 0.4)
            got = ia if actor else ic
            want = P.sample(pri, size, B, SEED, counter, actor)
            assert np.array_equal(got, want), (kind, counter, actor)
            t = P.targets(S, B, SEED, counter, actor)[b]
            k = int(got[b])
            assert prefix[k] > t and (k == 0 or prefix[k - 1] <= t) and pri[k] > 0
            if kind == "last":
                assert prefix[k] == t + 1
            else:
                assert prefix[k] - int(pri[k]) == t


def test_init_and_stamp(nav):
    from nav._lib import stream_handle
    s = stream_handle()
    cap = 3000
    st = Store(cap, np.full(cap, 123, np.int64))
    st.stat.fill_(-1)
    L = st.L
    L.nav_per_init(st.ref, s)
    assert not st.pri_host().any() and st.stat_host().tolist() == [P.ONE, 0, 0, 0]
    # a range that wraps the ring end
    L.nav_per_stamp(st.ref, 2900, 250, s)
    want = np.zeros(cap, np.int64)
    want[2900:] = P.ONE
    want[:150] = P.ONE
    assert np.array_equal(st.pri_host(), want)
    L.nav_per_stamp(st.ref, 17, 0, s)  # n = 0: nothing
    assert np.array_equal(st.pri_host(), want)
    # an update raises the running maximum; the next stamp hands it out
    idx = torch.tensor([5, 6], dtype=torch.int64, device=DEV)
    td = torch.tensor([30.0, 2.0], device=DEV)
    from nav._lib import ptr
    L.nav_per_update(st.ref, 2, ptr(idx), ptr(td), ptr(td), 0.6, 1e-6, s)
    q = P.priority(td.cpu().numpy(), td.cpu().numpy(), 0.6, 1e-6)
    top = st.stat_host()[0]
    assert abs(int(top) - int(q.max())) <= 1 and top > P.ONE
    L.nav_per_stamp(st.ref, 1000, 10, s)
    got = st.pri_host()
    assert (got[1000:1010] == top).all() and got[999] == 0 and got[1010] == 0
    L.nav_per_stamp(st.ref, 1234, cap, s)  # n = capacity: every row
    assert (st.pri_host() == top).all()
    assert st.stat_host().tolist() == [top, 0, 0, 0]


@pytest.mark.parametrize("alpha,eps", [(0.6, 1e-6), (2.0, 0.0), (1.0, 0.25)])
def test_update_duplicates_and_clamps(nav, alpha, eps):
    from nav._lib import ptr, stream_handle
    s = stream_handle()
    cap, rows, B = 3000, 50, 257
    g = torch.Generator().manual_seed(3)
    td1 = torch.randn(B, generator=g) * 5
    td2 = torch.randn(B, generator=g) * 5
    td1[:8] = torch.tensor([0.0, 0.0, 1e-30, 1e4, 1e4, -1e4, 1e-30, 0.0])
    td2[:8] = torch.tensor([0.0, 1e-30, 1e-30, 1e4, 0.0, -1e4, 3.0, 2.0])
    # every one of the 50 rows hit at least twice
    idx = torch.cat([torch.arange(rows), torch.arange(rows),
                     torch.randint(0, rows, (B - 2 * rows,), generator=g)])
    idx = idx[torch.randperm(B, generator=g)] + 1000
    assert np.bincount(idx.numpy() - 1000, minlength=rows).min() >= 2
    d1, d2 = td1.to(DEV), td2.to(DEV)
    # the device's own q per batch row: the same update on distinct rows
    one = Store(B)
    one.L.nav_per_init(one.ref, s)
    ar = torch.arange(B, dtype=torch.int64, device=DEV)
    one.L.nav_per_update(one.ref, B, ptr(ar), ptr(d1), ptr(d2), alpha, eps, s)
    q_dev = one.pri_host()
    q_ref = P.priority(td1.numpy(), td2.numpy(), alpha, eps)
    print(f"alpha {alpha} eps {eps}: max |q_dev - q_ref| {np.abs(q_dev - q_ref).max()}, "
          f"q in [{q_dev.min()}, {q_dev.max()}]")
    assert np.abs(q_dev - q_ref).max() <= 1
    assert q_dev.min() >= 1 and q_dev.max() <= MAXP
    assert one.stat_host()[0] == max(P.ONE, int(q_dev.max()))
    # duplicates: the maximum of the new values; the old value (larger than any of them) goes
    old = np.full(cap, MAXP, np.int64)
    st = Store(cap, old)
    st.stat[0] = 7
    st.L.nav_per_update(st.ref, B, ptr(idx.to(DEV)), ptr(d1), ptr(d2), alpha, eps, s)
    got = st.pri_host()
    assert np.array_equal(got, P.update(old, idx.numpy(), q_dev))
    assert np.abs(got - P.update(old, idx.numpy(), q_ref)).max() <= 1
    assert got.min() >= 1
    assert st.stat_host().tolist() == [int(q_dev.max()), 0, 0, 0]
    # twice the same call: the same store
    st.L.nav_per_update(st.ref, B, ptr(idx.to(DEV)), ptr(d1), ptr(d2), alpha, eps, s)
    assert np.array_equal(st.pri_host(), got)


def test_update_non_finite_errors_store_no_zero(nav):
    from nav._lib import ptr, stream_handle
    st = Store(8)
    s = stream_handle()
    st.L.nav_per_init(st.ref, s)
    td1 = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0], device=DEV)
    td2 = torch.tensor([1.0, 1.0, float("nan"), 0.0], device=DEV)
    idx = torch.arange(4, dtype=torch.int64, device=DEV)
    st.L.nav_per_update(st.ref, 4, ptr(idx), ptr(td1), ptr(td2), 0.6, 0.0, s)
    assert st.pri_host()[:4].tolist() == [1, MAXP, 1, 1]


# ---------------------------------------------------------------- the weighted critic kernel
SHAPES = [(64, 2), (256, 2), (200, 3)]


_SETUPS = {}


def _setup(hidden, nh, B):
    """mlp_ref.epoch_case on the device (nets, ring, injected idx and eps), built once."""
    key = (hidden, nh, B)
    if key not in _SETUPS:
        case = R.epoch_case(hidden, nh, B)
        _SETUPS.clear()  # one case's tensors at a time
        _SETUPS[key] = (case, *LN.device_epoch(case))
    return _SETUPS[key]


def _rows(nets, dev, B, **kw):
    """nav_td3_critic_rows (no w) or nav_td3_critic_rows_w into zeroed buffers."""
    return LN.critic_rows(nets, dev, B, fill=0.0, **kw)


def _flat_grads(nets, o, B):
    """nav_mlp_wgrad -> nav_grad_reduce of a rows launch: both critics' flat gradients."""
    return LN.flat_grads([nets["cr0"], nets["cr1"]], o, fill=0.0)


def _random_w(B, seed=0):
    g = torch.Generator().manual_seed(4000 + B + seed)
    return (1.0 - torch.rand(B, generator=g)).clamp_min(2.0 ** -20).to(DEV)  # (0, 1]


SAME_KEYS = ("dq", "es", "masks", "acts", "dz")
UNIT_CASES = [(h, nh, B) for h, nh in SHAPES for B in (100, 2150)] + [(64, 2, 2048)]


@pytest.mark.parametrize("hidden,nh,B", UNIT_CASES)
def test_unit_weights_equal_the_plain_launch(nav, hidden, nh, B):
    _, nets, dev = _setup(hidden, nh, B)
    plain = _rows(nets, dev, B)
    unit = _rows(nets, dev, B, w=torch.ones(B, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(plain["batch"], unit["batch"]) and torch.equal(plain["lp"], unit["lp"])
    for key in SAME_KEYS:
        for k in range(2):
            assert torch.equal(plain[key][k], unit[key][k]), (key, k)
    for k in range(2):
        td = unit["td"][k].cpu().numpy()
        assert np.isfinite(td).all() and (td >= 0).all() and td.max() > 0
        want = np.abs(plain["dq"][k].cpu().numpy().astype(np.float64)) * B / 2
        err = np.abs(td.astype(np.float64) - want) / np.spacing(td)
        print(f"hp {hidden} nh {nh} B {B} critic {k}: |td - |dq| B/2| max {err.max():.2f} ulp")
        assert err.max() <= (0 if B == 2048 else 2)


@pytest.mark.parametrize("hidden,nh", SHAPES)
@pytest.mark.parametrize("B", [100, 2150])
def test_random_weights(nav, hidden, nh, B):
    from nav._lib import descs, lib, parr, ptr, stream_handle
    L = lib()
    _, nets, dev = _setup(hidden, nh, B)
    cr = [nets["cr0"], nets["cr1"]]
    mid = cr[0].middle_layers()
    w = _random_w(B)
    plain = _rows(nets, dev, B)
    unit = _rows(nets, dev, B, w=torch.ones(B, device=DEV))
    wtd = _rows(nets, dev, B, w=w)
    fwd = _rows(nets, dev, B, w=w, row_backward=0)  # the Wo / bo partials alone
    # nav_mlp_backward of the weighted dq on the plain launch's masks: dz rows and W0 / bias
    # partials, into the forward-only launch's edge slabs
    udz = [torch.zeros(nh, B, cr[0].hp, device=DEV) for _ in range(2)]
    L.nav_mlp_backward(descs(*cr), 2, B, parr(*wtd["dq"]), 1, parr(*plain["masks"]),
                       ptr(plain["batch"]), 8, 0, None, parr(*udz), mid, None, parr(*fwd["es"]),
                       stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(plain["batch"], wtd["batch"])
    nblk = plain["lp"].shape[1]
    tm = (B + nblk - 1) // nblk
    tm = 32 if tm <= 32 else 64
    assert nblk == (B + tm - 1) // tm
    for k in range(2):
        assert torch.equal(wtd["dq"][k], plain["dq"][k] * w), k
        assert torch.equal(wtd["td"][k], unit["td"][k]), k
        assert torch.equal(wtd["masks"][k], plain["masks"][k]), k
        assert torch.equal(wtd["es"][k], fwd["es"][k]), k
        if mid:
            assert torch.equal(wtd["acts"][k], plain["acts"][k]), k
            assert torch.equal(udz[k][1:nh - 1], wtd["dz"][k][1:nh - 1]), k
        # each block's loss: an f32 sum of at most 64 non-negative terms
        e2 = wtd["td"][k].double().cpu() ** 2 * w.double().cpu()
        pad = torch.zeros(nblk * tm, dtype=torch.float64)
        pad[:B] = e2
        ref = pad.view(nblk, tm).sum(1)
        rel = ((wtd["lp"][k].double().cpu() - ref).abs() / ref).max().item()
        print(f"hp {hidden} nh {nh} B {B} critic {k}: loss_part rel err {rel:.2e}")
        assert rel <= 64 * 2.0 ** -24


@pytest.mark.parametrize("hidden,nh", SHAPES)
@pytest.mark.parametrize("B", [100, 2150])
def test_weighted_gradient_vs_fp64(nav, hidden, nh, B):
    """rows_w -> wgrad -> reduce with random weights against the fp64 weighted epoch, by
    mlp_ref's comparison and bars (as test_gpu_width_depth's unweighted critic epoch)."""
    case, nets, dev = _setup(hidden, nh, B)
    hp = nets["cr0"].hp
    w = _random_w(B, 1)
    o = _rows(nets, dev, B, w=w)
    grads = _flat_grads(nets, o, B)
    torch.cuda.synchronize()
    batch = case["rows"][case["idx"]]
    assert torch.equal(o["batch"].cpu(), batch)
    bits = [R.relu_bits(o["masks"][k], nh, hp, hidden, B) for k in range(2)]
    L = case["layers"]
    args = (L["ta"], [L["tc0"], L["tc1"]], [L["cr0"], L["cr1"]], batch, case["eps"], bits, w.cpu())
    ref, f32 = P.critic_epoch_w(*args), P.critic_epoch_w(*args, dtype=torch.float32)
    log, over = R.ParityLog(), []
    for k in range(2):
        R.assert_band_cap(*R.relu_band(L[f"cr{k}"], batch[:, :4], ref["zs"][k], bits[k]))
        scale = 2.0 / B * max(float(ref["q"][k].abs().max()), float(ref["y"].abs().max()))
        d = dict(dq=o["dq"][k].cpu(), loss=(o["lp"][k].double().sum() / B).reshape(1).cpu())
        d.update(R.flat_grad_tensors(grads[k].cpu(), 4, 1, hidden, hp, nh))
        # |q - y| is dq * B / 2 (before the weight): dq's scale times B / 2, a row quantity's bar
        d["td"] = o["td"][k].cpu()
        qr, qf = R.critic_quantities(ref, k), R.critic_quantities(f32, k)
        qr["td"], qf["td"] = ref["td"][k], f32["td"][k]
        over += log.judge(hp, nh, "critic_rows_w", R.compare(
            d, qr, qf, {"dq": scale, "td": scale * B / 2}))
    assert not over, over


@pytest.mark.parametrize("hidden,nh", SHAPES)
@pytest.mark.parametrize("B", [100, 2150])
def test_half_weights_halve_every_gradient(nav, hidden, nh, B):
    _, nets, dev = _setup(hidden, nh, B)
    plain = _rows(nets, dev, B)
    half = _rows(nets, dev, B, w=torch.full((B,), 0.5, device=DEV))
    gp, gh = _flat_grads(nets, plain, B), _flat_grads(nets, half, B)
    torch.cuda.synchronize()
    assert torch.equal(half["lp"], plain["lp"] * 0.5)
    for k in range(2):
        assert torch.equal(half["dq"][k], plain["dq"][k] * 0.5), k
        assert torch.equal(half["es"][k], plain["es"][k] * 0.5), k
        assert torch.equal(half["dz"][k], plain["dz"][k] * 0.5), k
        assert torch.equal(half["acts"][k], plain["acts"][k]), k
        assert torch.isfinite(gp[k]).all() and gp[k].abs().max() > 0
        assert torch.equal(gh[k], gp[k] * 0.5), k


@pytest.mark.parametrize("hidden,nh", SHAPES)
@pytest.mark.parametrize("row_backward", [0, 1])
def test_weighted_twin_forms_bit_identical(nav, hidden, nh, row_backward):
    B = 100
    _, nets, dev = _setup(hidden, nh, B)
    w = _random_w(B, 2)
    a = _rows(nets, dev, B, w=w, split=0, row_backward=row_backward)
    b = _rows(nets, dev, B, w=w, split=1, row_backward=row_backward)
    torch.cuda.synchronize()
    assert torch.equal(a["batch"], b["batch"]) and torch.equal(a["lp"], b["lp"])
    for key in SAME_KEYS + ("td",):
        for k in range(2):
            assert torch.equal(a[key][k], b[key][k]), (key, k)
    assert a["dq"][0].abs().max() > 0


# ---------------------------------------------------------------- the trainer
TRAINER = dict(n_envs=256, hidden=64, batch=128, replay_capacity=1024, envs_per_group=64)
PER = dict(per_alpha=0.6, per_beta=0.4, per_eps=1e-6)


def test_off_means_off(nav):
    from nav.trainer import VecTrainer
    snaps = []
    for kw in (dict(per_alpha=0.0), {}):
        tr = VecTrainer(device=DEV, **TRAINER, **kw)
        for _ in range(6):
            tr.step()
        torch.cuda.synchronize()
        assert tr.replay.pri is None and tr.replay.sums is None and tr.replay.stat is None
        assert tr.td3.per_launches == 0 and not tr.td3.per_on()
        assert not hasattr(tr.td3, "w_per")
        snaps.append(snapshot(tr, "env"))
        assert "per_alpha" not in tr.state_dict()["meta"]
    assert _same(*snaps)


@pytest.fixture(scope="module")
def per_run(nav):
    """A PER trainer: 4 collected ticks, then 4 single epochs, the store and the epoch's arrays
    recorded around each."""
    from nav.trainer import VecTrainer
    tr = VecTrainer(device=DEV, **TRAINER, **PER)
    for _ in range(4):
        tr.collect()
    torch.cuda.synchronize()
    ring = tr.replay
    host = lambda t: t.cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    rec = dict(stamped=host(ring.pri), stat0=host(ring.stat), epochs=[], seed=tr.seed)
    t = tr.td3
    for _ in range(4):
        e = dict(pri=host(ring.pri), counter=t.update_counter, size=len(ring))
        t.td3_update(ring, 1)
        torch.cuda.synchronize()
        e.update(idx_c=t.idx_c.cpu().numpy().copy(), idx_a=t.idx_a.cpu().numpy().copy(),
                 w=t.w_per.cpu().numpy().copy(), td1=t.td_abs1.cpu().numpy().copy(),
                 td2=t.td_abs2.cpu().numpy().copy(), after=host(ring.pri),
                 stat=host(ring.stat), params=_params(tr))
        rec["epochs"].append(e)
    return rec


def test_ticks_stamp_the_running_maximum(per_run):
    assert (per_run["stamped"] == P.ONE).all()  # 4 x 256 rows: the whole ring of 1 024
    assert per_run["stat0"].tolist() == [P.ONE, 0, 0, 0]


def test_first_epoch_is_plain(nav, per_run):
    """Every priority equals the stamp, so w == 1: a plain TD3 of the same seed, fed the PER
    run's indices, ends with the same bits."""
    from nav.trainer import VecTrainer
    e = per_run["epochs"][0]
    assert (e["w"] == np.float32(1.0)).all()
    tr = VecTrainer(device=DEV, **TRAINER)
    for _ in range(4):
        tr.collect()
    feed = iter([torch.from_numpy(e["idx_c"]).to(DEV), torch.from_numpy(e["idx_a"]).to(DEV)])
    tr.td3.td3_update(tr.replay, 1, idx_fn=lambda: next(feed))
    torch.cuda.synchronize()
    assert next(feed, None) is None
    assert _same(_params(tr), e["params"])


def test_epochs_follow_the_restatement(per_run):
    seed = per_run["seed"]
    for n, e in enumerate(per_run["epochs"]):
        B = e["idx_c"].shape[0]
        assert np.array_equal(e["idx_c"], P.sample(e["pri"], e["size"], B, seed, e["counter"],
                                                   False)), n
        assert np.array_equal(e["idx_a"], P.sample(e["pri"], e["size"], B, seed, e["counter"],
                                                   True)), n
        d = ulps(e["w"], P.weights(e["pri"], e["size"], e["idx_c"], PER["per_beta"]))
        q = P.priority(e["td1"], e["td2"], PER["per_alpha"], PER["per_eps"])
        want = P.update(e["pri"], e["idx_c"], q)
        dp = np.abs(e["after"] - want).max()
        print(f"epoch {n}: weight ulps {d.max()}, priority counts {dp}, "
              f"w in [{e['w'].min():.3f}, {e['w'].max():.3f}]")
        assert d.max() <= 1 and dp <= 1
        assert e["after"].min() >= 1
        assert e["stat"][1] == e["pri"][:e["size"]].min()
        before = int(per_run["epochs"][n - 1]["stat"][0]) if n else P.ONE
        assert abs(int(e["stat"][0]) - max(before, int(q.max()))) <= 1
    # the priorities moved, and with them the weights
    last = per_run["epochs"][-1]
    assert len(set(last["pri"].tolist())) > 2 and last["w"].min() < 1


def test_explicit_indices_win_and_still_update(nav):
    from nav.trainer import VecTrainer
    tr = VecTrainer(device=DEV, **TRAINER, **PER)
    for _ in range(4):
        tr.collect()
    g = torch.Generator().manual_seed(1)
    ic = torch.randint(0, 1024, (128,), generator=g).to(DEV)
    ia = torch.randint(0, 1024, (128,), generator=g).to(DEV)
    feed = iter([ic, ia])
    tr.td3.td3_update(tr.replay, 1, idx_fn=lambda: next(feed))
    torch.cuda.synchronize()
    pri = tr.replay.pri.cpu().numpy().view(np.uint32).astype(np.int64)
    q = P.priority(tr.td3.td_abs1.cpu().numpy(), tr.td3.td_abs2.cpu().numpy(), PER["per_alpha"],
                   PER["per_eps"])
    want = P.update(np.full(1024, P.ONE, np.int64), ic.cpu().numpy(), q)
    assert np.abs(pri - want).max() <= 1
    # the plain learner on the same indices: w == 1, the same parameters
    pl = VecTrainer(device=DEV, **TRAINER)
    for _ in range(4):
        pl.collect()
    feed = iter([ic, ia])
    pl.td3.td3_update(pl.replay, 1, idx_fn=lambda: next(feed))
    torch.cuda.synchronize()
    assert _same(_params(pl), _params(tr))


def test_checkpoint_resume_with_priorities(nav, tmp_path):
    from nav.trainer import VecTrainer
    a = VecTrainer(device=DEV, **TRAINER, **PER)
    for _ in range(5):
        a.step()
    path = os.path.join(tmp_path, "per.pt")
    a.save(path)
    b = VecTrainer.load(path, device=DEV)
    assert b.td3.per_on() and b.replay.pri is not None
    c = b.td3.cfg
    assert (c.per_alpha, c.per_beta, c.per_eps) == (0.6, 0.4, 1e-6)
    assert torch.equal(a.replay.pri, b.replay.pri) and torch.equal(a.replay.stat, b.replay.stat)
    assert len(set(a.replay.pri.cpu().tolist())) > 2
    for _ in range(3):
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert _same(_params(a), _params(b))
    assert torch.equal(a.replay.rows, b.replay.rows)
    assert torch.equal(a.replay.pri, b.replay.pri) and torch.equal(a.replay.stat, b.replay.stat)
    for k in a.ENV_STATE:
        assert torch.equal(getattr(a.env, k), getattr(b.env, k)), k
    # a checkpoint without the per_* entries loads as PER off
    plain = VecTrainer(device=DEV, demos=False, **TRAINER)
    plain.step()
    off = VecTrainer.from_state_dict(plain.state_dict(), device=DEV)
    assert not off.td3.per_on() and off.replay.pri is None


class _Hook:
    world_size = 1

    def __call__(self, bucket):
        return None


@pytest.mark.parametrize("kw", [dict(demo_fraction=0.25), dict(bc_weight=1.0),
                                dict(demo_fraction=0.25, bc_weight=1.0),
                                dict(grad_hook=_Hook()), dict(overlap_collect=True)],
                         ids=["demo_fraction", "bc_weight", "both", "grad_hook", "overlap_collect"])
def test_rejected_combinations(nav, kw):
    from nav.trainer import VecTrainer
    with pytest.raises(ValueError, match="prioritised replay"):
        VecTrainer(device=DEV, demos=False, **TRAINER, **PER, **kw)


def test_rejected_population_member_and_bad_alpha(nav):
    from nav.population import PopulationTrainer
    from nav.trainer import VecTrainer
    with pytest.raises(ValueError, match="prioritised replay"):
        PopulationTrainer([{}, {"per_alpha": 0.6}], envs_per_member=64, hidden=64, batch=64,
                          envs_per_group=64, demos=False, device=DEV)
    with pytest.raises(ValueError, match="per_alpha"):
        VecTrainer(device=DEV, demos=False, per_alpha=-0.5, **TRAINER)


def test_ring_without_priorities_refuses_a_per_learner(nav):
    from nav import config as K
    from nav.td3 import TD3
    from nav.vec_env import ReplayRing
    t = TD3(K.TD3Config(batch_size=64, net=K.NetConfig(hidden=64, n_hidden=2), per_alpha=0.6),
            device=DEV)
    ring = ReplayRing(256, DEV)
    ring.advance(256)
    with pytest.raises(ValueError, match="priorities"):
        t.td3_update(ring, 1)


# ---------------------------------------------------------------- the workspace key
def _filled_ring():
    """512 seeded rows with priorities (every row stamped) and cut marks, stride 64."""
    from nav.vec_env import ReplayRing
    g = torch.Generator().manual_seed(7)
    ring = ReplayRing(512, DEV, priorities=True, cuts=True)
    ring.rows.copy_(torch.randn(512, 8, generator=g))
    ring.rows[:, 7] = (torch.rand(512, generator=g) < 0.05).float()
    ring.cut.copy_((torch.rand(512, generator=g) < 0.1).to(torch.uint8))
    ring.stamp(ring.advance(512), 512)
    ring.stride = 64
    return ring


@pytest.mark.parametrize("field,value", [("per_alpha", 0.6), ("n_step", 3)])
def test_a_mode_switched_on_later_gets_its_workspace(nav, field, value):
    """The workspace is keyed by what it allocates for. A: a learner built with the mode off runs
    2 epochs, has the mode switched on in its config and runs 2 more. B: a learner built with the
    mode on takes A's state and ring priorities of that moment and runs 2 epochs. Equal state
    and equal ring priorities, bit for bit."""
    from nav import config as K
    from nav.td3 import TD3
    cfg = lambda **kw: K.TD3Config(batch_size=64, net=K.NetConfig(hidden=64, n_hidden=2),  # noqa: E731
                                   **kw)
    ring_a, ring_b = _filled_ring(), _filled_ring()
    a = TD3(cfg(), device=DEV)
    a.td3_update(ring_a, 2)
    assert not hasattr(a, "w_per") and not hasattr(a, "staged")
    torch.cuda.synchronize()
    mid = a.state_dict()
    ring_b.pri.copy_(ring_a.pri)
    ring_b.stat.copy_(ring_a.stat)
    setattr(a.cfg, field, value)
    a.td3_update(ring_a, 2)
    b = TD3(cfg(**{field: value}), device=DEV)
    b.load_state_dict(mid)
    b.td3_update(ring_b, 2)
    torch.cuda.synchronize()
    assert a.per_launches == b.per_launches == (6 if field == "per_alpha" else 0)
    assert a.nstep_launches == b.nstep_launches == (2 if field == "n_step" else 0)
    assert _same(a.state_dict(), b.state_dict()) and not _same(mid, b.state_dict())
    assert torch.equal(ring_a.pri, ring_b.pri) and torch.equal(ring_a.stat, ring_b.stat)
    assert (field == "per_alpha") == (len(set(ring_a.pri.cpu().tolist())) > 2)
