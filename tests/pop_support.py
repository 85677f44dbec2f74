"""Learners, rings, test-episode inputs and state trees the GPU test modules share: one copy of
each. Where two modules' helpers of one name covered different things, the function here takes a
parameter that reproduces each caller (said at the parameter); comparisons are bitwise."""
import ctypes as C

import numpy as np
import torch

DEV = "cuda"
CAP, FILL = 4096, 3000  # make_ring's capacity and fill
SOA = ("state", "goal", "region", "hist", "meta", "plan_index", "path_length", "episodes",
       "noise_scale")
NETS = ("actor", "critic1", "critic2", "target_actor", "target_critic1", "target_critic2")


# ---- trees of dicts / lists / tensors / values
def differences(a, b, path="", out=None):
    """The paths at which two trees of dicts / tensors / values differ (bitwise; a tensor may be
    on the host on one side and on the device on the other). Differing key sets or lengths are
    asserted, not reported."""
    out = [] if out is None else out
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            differences(a[k], b[k], f"{path}/{k}", out)
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            differences(x, y, f"{path}/{i}", out)
    elif torch.is_tensor(a):
        if not (torch.equal(a, b) if a.device == b.device else torch.equal(a.cpu(), b.cpu())):
            out.append(path)
    elif a != b:
        out.append(path)
    return out


def equal_tree(a, b, path=""):
    bad = differences(a, b, path)
    assert not bad, bad


def same(a, b):
    return not differences(a, b)


def leaves(tree, path=""):
    if isinstance(tree, dict):
        for k, v in tree.items():
            yield from leaves(v, f"{path}/{k}")
    else:
        yield path, tree


# ---- lone learners and their rings
def make_td3(m, hidden, nh, B, epochs, splits=None, seed=None, **cfg):
    """Member m's learner: its own seed (weights, sampling, smoothing noise; 1000 + 17 m unless
    given) and its own value of every per-member hyper-parameter; cfg: further TD3Config fields,
    which win."""
    from nav import config as K
    from nav.td3 import TD3
    kw = dict(actor_lr=1e-4 * (m + 1), critic_lr=1e-3 / (m + 1), gamma=0.99 - 0.01 * m,
              tau=0.005 * (m + 1), policy_noise=0.2 + 0.05 * m, noise_clip=0.5 - 0.05 * m,
              policy_update_delay=2, max_action=5.0 - 0.5 * m, batch_size=B, num_epochs=epochs,
              net=K.NetConfig(hidden=hidden, n_hidden=nh))
    kw.update(cfg)
    return TD3(K.TD3Config(**kw), device=DEV, seed=1000 + 17 * m if seed is None else seed,
               wgrad_splits=splits)


def make_ring(m, tail=0, storage=None, cap=CAP, fill=FILL):
    """A ring of `cap` rows filled to `fill`: fixed random rows (done in {0, 1}), the unfilled
    rows zero. tail: that many demonstration rows behind it (done = 0, every row times 10, as
    test_gpu_population_bc's rings); storage: the rows to use instead."""
    from nav.vec_env import ReplayRing
    if storage is None:
        g = torch.Generator().manual_seed(500 + m)
        storage = torch.randn(cap + tail, 8, generator=g) * (10 if tail else 1)
        storage[:, 7] = (torch.rand(cap + tail, generator=g) < 0.1).float()
        storage[fill:cap] = 0.0
        storage[cap:, 7] = 0.0
    r = ReplayRing(cap, DEV, tail=tail)
    r.storage.copy_(storage.to(DEV))
    r.advance(fill)
    return r


def injection(m, B):
    g = torch.Generator().manual_seed(900 + m)
    ic = torch.randint(0, FILL, (B,), generator=g, dtype=torch.int64).to(DEV)
    ia = torch.randint(0, FILL, (B,), generator=g, dtype=torch.int64).to(DEV)
    eps = torch.randn(B, 2, generator=g).to(DEV)
    return ic, ia, eps


def _clone(x):
    return x.detach().clone()


def _optimizers(t):
    return {"actor": t.actor_optimizer, "critic1": t.critic_optimizer_1,
            "critic2": t.critic_optimizer_2}


def copied_state(t):
    """What an exploit pair copies apart from the ring, as device clones."""
    nets, opts = t.networks(), _optimizers(t)
    return {"params": {k: _clone(nets[k].params) for k in NETS},
            "packed": {k: _clone(nets[k].packed) for k in NETS},
            "m": {k: _clone(o.m) for k, o in opts.items()},
            "v": {k: _clone(o.v) for k, o in opts.items()}}


def workspace(t):
    return {k: _clone(getattr(t, a)) for k, a in (
        ("batch", "batch"), ("batch2", "batch2"), ("dq1", "dq1"), ("dq2", "dq2"), ("da", "da"),
        ("q", "q1"), ("loss_part", "loss_part"), ("grad_a", "grad_a"), ("grad_c", "grad_c"),
        ("eslab1", "eslab1"), ("hslab", "hslab"))}


def learner_state(t, work=False):
    """A learner's nets (parameters, packed images), Adam moments and step counts, both sampled
    batches, dq, loss_part, q, da and the update counter, as device clones. work: workspace() as
    well, the gradient and slab buffers included (test_gpu_pbt's form: a buffer an exploit missed
    would show; a batched member's slabs need not equal a lone learner's)."""
    nets = t.networks()
    s = {"params": {k: _clone(v.params) for k, v in nets.items()},
         "packed": {k: _clone(v.packed) for k, v in nets.items()},
         "adam": {k: {"m": _clone(o.m), "v": _clone(o.v), "t": o.step_count}
                  for k, o in _optimizers(t).items()},
         "batch": _clone(t.batch), "batch2": _clone(t.batch2), "dq1": _clone(t.dq1),
         "dq2": _clone(t.dq2), "loss_part": _clone(t.loss_part), "q": _clone(t.q1),
         "da": _clone(t.da), "update_counter": t.update_counter}
    if work:
        s["work"] = workspace(t)
    return s


def state_member(t, ring):
    """The learner state of one TD3 and its ring as a nav_td3_member; everything else null. The
    tests' own restatement, independent of nav.population.state_member."""
    from nav._lib import NavTd3Member
    e = NavTd3Member()
    e.actor, e.target_actor = t.actor_network.desc(), t.target_actor.desc()
    e.critics[0], e.critics[1] = t.critic_network_1.desc(), t.critic_network_2.desc()
    e.target_critics[0] = t.target_critic_network_1.desc()
    e.target_critics[1] = t.target_critic_network_2.desc()
    e.replay = ring.desc()
    oa, oc1, oc2 = t.actor_optimizer, t.critic_optimizer_1, t.critic_optimizer_2
    e.m_actor, e.v_actor = oa.m.data_ptr(), oa.v.data_ptr()
    e.m_critic[0], e.m_critic[1] = oc1.m.data_ptr(), oc2.m.data_ptr()
    e.v_critic[0], e.v_critic[1] = oc1.v.data_ptr(), oc2.v.data_ptr()
    return e


def member_state(tr, m, tail=False):
    """Everything member m's next step reads, as host tensors: its env slice, its ring (tail: with
    the demonstration tail behind it) and its learner (every parameter, Adam moment and
    counter)."""
    sl = tr.member_slice(m)
    env = {k: (getattr(tr.env, k)[:, sl] if k == "hist" else getattr(tr.env, k)[sl]).cpu()
           for k in SOA}
    r = tr.rings[m]
    rows = r.storage if tail else r.rows
    return {"env": env, "replay": {"rows": rows.cpu(), "position": r.position, "size": r.size},
            "td3": tr.td3[m].state_dict(), "steps": tr.steps}


# ---- a lone trainer's state, flat
def params(t):
    """{name: params clone} of a TD3's (or a trainer's learner's) six nets."""
    return {k: n.params.clone() for k, n in getattr(t, "td3", t).networks().items()}


def moments(t):
    out = {}
    for k, o in _optimizers(getattr(t, "td3", t)).items():
        out[k + "_m"], out[k + "_v"] = o.m.clone(), o.v.clone()
    return out


def snapshot(tr, *parts, ring="rows"):
    """A VecTrainer's parameters and its ring (`ring`: "rows", or "storage" with the tail) under
    "ring", plus the named parts: "moments", "env" (every ENV_STATE tensor), "packed" (the nets'
    images, as <net>_packed) and "action". Each caller names what its comparison covered."""
    assert set(parts) <= {"moments", "env", "packed", "action"}, parts
    s = params(tr)
    s["ring"] = getattr(tr.replay, ring).clone()
    if "moments" in parts:
        s.update(moments(tr))
    if "env" in parts:
        s.update({k: getattr(tr.env, k).clone() for k in tr.ENV_STATE})
    if "packed" in parts:
        s.update({k + "_packed": n.packed.clone() for k, n in tr.td3.networks().items()})
    if "action" in parts:
        s["action"] = tr.action.clone()
    return s


# ---- test episodes: fields, actors, starts and the composition nav_test_rollout fuses
def random_field(seed):
    rng = np.random.default_rng(seed)
    speed = rng.uniform(0.05, 0.95, (100, 100)).astype(np.float32)  # in (0, 1)
    angle = rng.uniform(0.0, 1.0, (100, 100)).astype(np.float32)    # in [0, 1]
    return speed, angle


def make_actor(hidden, nh, seed):
    """(the actor on the device, its layers as CPU tensors)."""
    from nav.mlp import DeviceMLP
    from oracle.td3_oracle import make_mlp_params
    p = make_mlp_params(seed, [2] + [hidden] * nh + [2])
    return DeviceMLP(2, 2, hidden, nh, DEV).load(p), [(torch.tensor(W), torch.tensor(b))
                                                      for W, b in p]


def make_env(n, speed, angle, **overrides):
    from nav.vec_env import VecEnv, make_field
    return VecEnv(n, make_field(speed, angle, DEV), seed=77, demo_flag=False, device=DEV,
                  **overrides)


def random_starts(env, seed):
    """Uniform starts in the world; every 5th env one unit from its goal, so that some rows stop
    at the first step while their tile goes on."""
    g = torch.Generator().manual_seed(seed)
    st = torch.rand(env.n, 2, generator=g, dtype=torch.float64) * 98.0
    near = torch.arange(env.n) % 5 == 0
    st[near] = env.goal.cpu()[near] + torch.tensor([0.6, -0.8], dtype=torch.float64)
    return st.clamp_(0.0, 98.0).to(DEV)


def clone_out(out):
    return {k: v.clone() for k, v in out.items()}


def norm2_rows(orc, d):
    """orc.norm2 (sqrt(fma(y, y, x * x)), the device's norm2) of every row of d [k][2]."""
    return np.array([orc.norm2(x, y) for x, y in d.tolist()], np.float64).reshape(len(d))


def unfused_episode(orc, env, actor, start, T):
    """The composition the kernel fuses: per step nav_act(mode=1) then nav_env_step on a scratch
    VecEnv, stopped rows masked back, the stop test on the CPU with the oracle's norm2."""
    from nav._lib import lib, ptr, stream_handle
    from nav.vec_env import VecEnv
    n = env.n
    sc = VecEnv(n, env.field, device=DEV, init=False)
    sc.goal.copy_(env.goal)
    sc.state.copy_(start)
    thr = env.p.goal_threshold
    goal = env.goal.cpu().numpy()
    action = torch.zeros(n, 2, dtype=torch.float64, device=DEV)
    d = actor.desc()
    run = np.ones(n, bool)
    reached = np.zeros(n, np.uint8)
    steps = np.full(n, T, np.int32)
    best = np.full(n, np.inf)
    traj = torch.zeros(T, n, 2, dtype=torch.float64, device=DEV)
    for t in range(1, T + 1):
        prev = sc.state.clone()
        lib().nav_act(C.byref(sc.p), C.byref(d), n, ptr(sc.state), ptr(sc.goal), None, None, 0, 1,
                      ptr(action), None, stream_handle())
        sc.step(action)
        keep = torch.from_numpy(~run).to(DEV)
        sc.state.copy_(torch.where(keep[:, None], prev, sc.state))
        traj[t - 1] = sc.state
        s = sc.state.cpu().numpy()
        idx = np.nonzero(run)[0]
        dist = norm2_rows(orc, s[idx] - goal[idx])
        best[idx] = np.minimum(best[idx], dist)
        hit = idx[dist <= thr]
        reached[hit] = 1
        steps[hit] = t
        run[hit] = False
    return {"traj": traj, "final_state": sc.state.clone(), "reached": torch.from_numpy(reached),
            "steps": torch.from_numpy(steps), "best_distance": torch.from_numpy(best)}


# ---- two learners on one ring (tests/test_gpu_shared_policy.py and the full-size tests)
def replay_rows(n, seed):
    """Replay rows shaped like the tick's (robot.py:79-96): s in the world, clipped actions,
    goal + demo-shaped rewards, s' = a step away, ~2 % dones."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 98.9999, (n, 2))
    a = rng.uniform(-5, 5, (n, 2))
    s2 = np.clip(s + 0.8 * a, 0, 98.9999)
    goal = rng.uniform(5, 95, (n, 2))
    r = -np.linalg.norm(s2 - goal, axis=1) - 10 * rng.uniform(0, 5, n)
    d = (rng.uniform(size=n) < 0.02).astype(np.float64)
    return np.concatenate([s, a, r[:, None], s2, d[:, None]], 1).astype(np.float32)


def make_learner(B, hidden, nh, params):
    from nav import config as K
    from nav.mlp import DeviceMLP
    from nav.td3 import TD3
    pa, p1, p2 = params
    mk = lambda di, do, p: DeviceMLP(di, do, hidden, nh, DEV).load(p)  # noqa: E731
    cfg = K.TD3Config(batch_size=B, num_epochs=2, net=K.NetConfig(hidden=hidden, n_hidden=nh))
    return TD3(cfg, DEV, actor=mk(2, 2, pa), critic1=mk(4, 1, p1), critic2=mk(4, 1, p2))


def ring_of(rows):
    from nav.vec_env import ReplayRing
    rep = ReplayRing(len(rows), DEV)
    rep.rows.copy_(torch.tensor(rows))
    rep.size = len(rows)
    return rep
