"""The learner's modes, host side: every row of TD3Config's rule table refuses at every entry point
that can meet it (the config's check, the learner, the trainer, the population trainer) before any
device work; every built combination passes; the checkpoint meta's mode keys and their way back
into keywords; and the replay ring's half of the ring contract. No GPU and no library call."""
import pytest

B = 128
BC = dict(demo_fraction=0.25, bc_weight=1.0)
PER = dict(per_alpha=0.6)


class _Hook:
    world_size = 1

    def __call__(self, bucket):
        return None


HOOK = _Hook()
# (id, the mode fields, what the entry point runs with, the message's fragment): one per row of
# TD3Config._rules, then b_demo()'s three
ROWS = [
    ("n_step_range", dict(n_step=17), {}, "n_step must be an int"),
    ("per_alpha_range", dict(per_alpha=-1.0), {}, "per_alpha must be >= 0"),
    ("population_per", PER, dict(population="members"), "prioritised replay"),
    ("population_n_step", dict(n_step=3), dict(population="members"), "multi-step returns"),
    ("batched_q_filter", dict(bc_q_filter=True, **BC), dict(population="batched"), "bc_q_filter"),
    ("n_step_bc", dict(n_step=3, **BC), {}, "multi-step returns"),
    ("n_step_hook", dict(n_step=3), dict(grad_hook=HOOK), "multi-step returns"),
    ("n_step_overlap", dict(n_step=3), dict(overlap_collect=True), "multi-step returns"),
    ("per_bc", dict(**PER, **BC), {}, "prioritised replay"),
    ("per_hook", PER, dict(grad_hook=HOOK), "prioritised replay"),
    ("per_overlap", PER, dict(overlap_collect=True), "prioritised replay"),
    ("demo_fraction_range", dict(demo_fraction=1.5), {}, "demo_fraction must lie"),
    ("bc_weight_without_rows", dict(bc_weight=1.0), {}, "bc_weight needs"),
    ("q_filter_alone", dict(bc_q_filter=True), {}, "bc_q_filter"),
]


def rows(*without):
    """The rows an entry point can meet: those whose context it takes."""
    return pytest.mark.parametrize(
        "fields,ctx,fragment", [r[1:] for r in ROWS if not set(r[2]) & set(without)],
        ids=[r[0] for r in ROWS if not set(r[2]) & set(without)])


@pytest.fixture
def no_device(monkeypatch):
    """Whatever a constructor does first on the device raises AssertionError: a ValueError that
    arrives all the same was raised before it, on any machine."""
    import nav.mlp
    import nav.population
    import nav.trainer

    def touched(*a, **kw):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(nav.trainer, "make_field_device", touched)
    monkeypatch.setattr(nav.trainer, "make_env", touched)
    monkeypatch.setattr(nav.population, "make_field_device", touched)
    monkeypatch.setattr(nav.population, "make_env", touched)
    monkeypatch.setattr(nav.mlp.DeviceMLP, "__init__", touched)


def _cfg(**fields):
    from nav import config as K
    return K.TD3Config(batch_size=B, net=K.NetConfig(hidden=64, n_hidden=2), **fields)


# ---- (a) every row, at every entry point
@rows()
def test_check_refuses(fields, ctx, fragment):
    with pytest.raises(ValueError, match=fragment):
        _cfg(**fields).check(**ctx)


@rows("overlap_collect", "population")
def test_learner_refuses_before_it_allocates(no_device, fields, ctx, fragment):
    from nav.td3 import TD3
    with pytest.raises(ValueError, match=fragment):
        TD3(_cfg(**fields), device="cuda", **ctx)


@rows("population")
def test_trainer_refuses_before_it_builds(no_device, fields, ctx, fragment):
    from nav.trainer import VecTrainer
    with pytest.raises(ValueError, match=fragment):
        VecTrainer(n_envs=256, hidden=64, batch=B, **fields, **ctx)


@rows("grad_hook", "overlap_collect")
def test_population_refuses_before_it_builds(no_device, fields, ctx, fragment):
    from nav.population import PopulationTrainer
    with pytest.raises(ValueError, match=fragment) as e:
        PopulationTrainer([{}, dict(fields)], envs_per_member=64, hidden=64, batch=B,
                          envs_per_group=64, learner=ctx.get("population", "members"))
    assert "member 1" in str(e.value)


def test_the_hook_contract_and_the_demonstrations_come_first_too(no_device):
    from nav.population import PopulationTrainer
    from nav.td3 import TD3
    from nav.trainer import VecTrainer
    with pytest.raises(ValueError, match="world_size"):
        TD3(_cfg(), device="cuda", grad_hook=lambda bucket: None)
    with pytest.raises(ValueError, match="demos=True"):
        VecTrainer(n_envs=256, hidden=64, batch=B, demos=False, **BC)
    with pytest.raises(ValueError, match="demos=True"):
        PopulationTrainer([{}, BC], envs_per_member=64, hidden=64, batch=B, envs_per_group=64,
                          demos=False)
    with pytest.raises(TypeError, match="n_steps"):
        VecTrainer(n_envs=256, hidden=64, batch=B, n_steps=3)


def test_a_bare_learner_meets_the_same_rule_in_the_population_learner():
    """PopulationLearner._bc_members' guard is the table's row, the member named."""
    with pytest.raises(ValueError, match=r"bc_q_filter.*member 2"):
        _cfg(bc_q_filter=True, **BC).check(population="batched", member=2)
    with pytest.raises(ValueError, match=r"member 0.*bc_q_filter"):
        _cfg(bc_q_filter=True).check(population="members", member=0)


def test_the_older_entries_give_what_they_gave():
    assert _cfg(**BC).b_demo() == 32 and _cfg().b_demo() == 0
    _cfg(bc_weight=1.0, n_step=1).check_n_step()  # only the rows that name n_step
    _cfg(per_alpha=-1.0).check_n_step()
    with pytest.raises(ValueError, match="multi-step returns"):
        _cfg(n_step=3).check_n_step(HOOK)
    c = _cfg(bc_q_filter=True)
    assert c.bc_on() and not c.per_on() and not c.nstep_on()
    assert _cfg(**PER).per_on() and _cfg(n_step=2).nstep_on() and not _cfg().bc_on()


# ---- (b) every combination that is built
VALID = [("plain", {}, None), ("bc", BC, None), ("bc_q_filter", dict(bc_q_filter=True, **BC), None),
         ("per", PER, None), ("n_step", dict(n_step=3), None),
         ("per_n_step", dict(n_step=3, **PER), None), ("plain_hook", {}, HOOK),
         ("bc_hook", BC, HOOK)]
valid = pytest.mark.parametrize("fields,hook", [v[1:] for v in VALID], ids=[v[0] for v in VALID])


@valid
def test_valid_combinations_pass(fields, hook):
    _cfg(**fields).check(grad_hook=hook)
    if hook is None and not _cfg(**fields).per_on() and not _cfg(**fields).nstep_on():
        _cfg(**fields).check(population="members", member=3)


# ---- (c) the checkpoint meta's mode keys
ALWAYS = {"demo_fraction", "bc_weight", "q_weight"}


@valid
def test_meta_keys_and_the_way_back(fields, hook):
    from nav import config as K
    c = _cfg(**fields)
    meta = K.mode_meta(c)
    want = set(ALWAYS)
    if "per_alpha" in fields:
        want |= {"per_alpha", "per_beta", "per_eps"}
    if "n_step" in fields:
        want.add("n_step")
    if "bc_q_filter" in fields:
        want.add("bc_q_filter")
    assert set(meta) == want and all(meta[k] == getattr(c, k) for k in meta)
    back = K.mode_kwargs({"n_envs": 256, "steps": 7, **meta})
    assert back == {k: getattr(c, k) for k in K.MODE_FIELDS} and list(back) == list(K.MODE_FIELDS)
    assert all(type(back[k]) is type(getattr(c, k)) for k in back)


def test_an_old_checkpoint_loads_as_all_defaults():
    from nav import config as K
    old = {"n_envs": 256, "seed": 1, "envs_per_group": 64, "hidden": 64, "n_hidden": 2,
           "batch": B, "updates_per_step": 2, "steps": 7}
    d = K.TD3Config()
    assert K.mode_kwargs(old) == {k: getattr(d, k) for k in K.MODE_FIELDS}
    assert K.MODE_FIELDS == ("demo_fraction", "bc_weight", "q_weight", "bc_q_filter", "per_alpha",
                             "per_beta", "per_eps", "n_step")
    # a non-default per_beta survives only with the mode on, as the meta has always had it
    assert "per_beta" not in K.mode_meta(_cfg(per_beta=0.7))
    assert K.mode_kwargs(K.mode_meta(_cfg(per_beta=0.7, **PER)))["per_beta"] == 0.7


# ---- (d) the ring contract
def test_ring_needs_and_check_serves():
    from nav.vec_env import ReplayRing, ring_needs
    assert ring_needs(_cfg()) == dict(tail=False, priorities=False, cuts=False)
    assert ring_needs(_cfg(**BC)) == dict(tail=True, priorities=False, cuts=False)
    assert ring_needs(_cfg(n_step=3, **PER)) == dict(tail=False, priorities=True, cuts=True)
    plain = ReplayRing(64, "cpu")
    plain.check_serves(_cfg())
    for fields, fragment in ((BC, "demonstration tail"), (PER, "priorities"),
                             (dict(n_step=3), "cut marks")):
        with pytest.raises(ValueError, match=fragment):
            plain.check_serves(_cfg(**fields))
    plain.check_serves(_cfg(**BC), injected=True)  # the caller's indices address the rows
    plain.check_serves(_cfg(demo_fraction=0.001))  # rounds to no demonstration row
    cuts = ReplayRing(64, "cpu", cuts=True)
    with pytest.raises(ValueError, match="stride"):
        cuts.check_serves(_cfg(n_step=3))
    cuts.stride = 16
    cuts.check_serves(_cfg(n_step=3))
    ReplayRing(64, "cpu", tail=8).check_serves(_cfg(**BC))
