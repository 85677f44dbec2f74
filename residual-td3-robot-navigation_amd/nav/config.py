"""Constants and hyper-parameters of the reference, in one place.

constants.py:6-53 (world, action bound, CEM sizes, costs, test threshold), configuration.py:26 (seed)
and robot.py:21-54 (demo augmentation, path length, exploration, replay, reward shaping, TD3).
"""
from dataclasses import dataclass, field

from ._abi import parse_header

# constants.py
WORLD_SIZE = 100
ROBOT_MAX_ACTION = 5
INIT_REGION_SIZE = 25
UPDATE_RATE = 10
DEMOS_CEM_NUM_ITERATIONS = 4
DEMOS_CEM_NUM_PATHS = 100
DEMOS_CEM_PATH_LENGTH = 200
DEMOS_CEM_NUM_ELITES = 10
STARTING_MONEY = 100
COST_PER_STEP = 0.01
COST_PER_CPU_SECOND = 0.03
COST_PER_DEMO = 20
COST_PER_RESET = 5
TEST_DISTANCE_THRESHOLD = 5
TEST_TIMEOUT = 100

# configuration.py
RANDOM_SEED = 1707366464

# robot.py:21-54
NUM_DEMO = 3
NUM_AUGMENTS = 3
AUG_NOISE = 2.5
AUG_INTERPOLATION = 5
PATH_LENGTH = 50
PATH_INCREASE = 20
INITIAL_NOISE = 1
NOISE_DECAY = 0.75
BUFFER_SIZE = 10000
STUCK_THRESHOLD = 2
STUCK_STEPS = 5
STUCK_PENALTY = 50
GOAL_REWARD = 50
DEMO_PROXIMITY_FACTOR = 10
ACTOR_LR = 0.00001
CRITIC_LR = 0.00001
POLICY_UPDATE_DELAY = 2
TARGET_POLICY_NOISE = 0.2
NOISE_CLIP = 0.5
TD3_EPOCHS = 100
TD3_BATCH_SIZE = 100
GAMMA = 0.99
TAU = 0.001

# include/navenv.h
NSTEP_MAX = parse_header()[0]["NAV_NSTEP_MAX"]  # the longest multi-step return


@dataclass
class NetConfig:
    """Actor / critic width: 3 x 200 is the reference (robot.py:145-148, 185-188); 2 x 256 is the
    BASELINE config-3 throughput shape."""
    hidden: int = 200
    n_hidden: int = 3

    @property
    def hidden_pad(self):
        return (self.hidden + 31) // 32 * 32


@dataclass
class TD3Config:
    actor_lr: float = ACTOR_LR
    critic_lr: float = CRITIC_LR
    gamma: float = GAMMA
    tau: float = TAU
    policy_noise: float = TARGET_POLICY_NOISE
    noise_clip: float = NOISE_CLIP
    policy_update_delay: int = POLICY_UPDATE_DELAY
    max_action: float = ROBOT_MAX_ACTION
    batch_size: int = TD3_BATCH_SIZE
    num_epochs: int = TD3_EPOCHS
    # learning from demonstrations (off by default): the actor's loss is -q_weight * mean Q +
    # bc_weight * (behaviour-cloning term on the batch's demonstration rows), and demo_fraction
    # of every batch is drawn from the demonstration tail behind the replay ring
    bc_weight: float = 0.0
    q_weight: float = 1.0
    demo_fraction: float = 0.0
    # the Q-filter of the BC term (Nair et al. 2018; off by default): a demonstration row adds its
    # BC term only where online critic 1 rates its action above the policy's, Q1(s, a) >
    # Q1(s, pi(s)), strictly; the term's normaliser stays the batch's demonstration rows
    bc_q_filter: bool = False
    # prioritised replay (off by default, per_alpha == 0): batches are drawn in proportion to
    # priority (|TD error| + per_eps)^per_alpha and the critics' loss carries the importance
    # weights (N p_k / S)^-per_beta over their maximum; per_beta is read every epoch
    per_alpha: float = 0.0
    per_beta: float = 0.4
    per_eps: float = 1e-6
    # multi-step returns (off by default, n_step == 1): the critics' target is
    # r_t + ... + gamma^(k-1) r_{t+k-1} + gamma^k min Q'(s_{t+k}, a') with k <= n_step, cut short
    # where the env was reset or the ring's write head is reached (1 .. NAV_NSTEP_MAX = 16)
    n_step: int = 1
    net: NetConfig = field(default_factory=NetConfig)

    def bc_on(self):
        # (bc_q_filter alone counts as on, so that b_demo() refuses it)
        return self.demo_fraction != 0 or self.bc_weight != 0 or self.bc_q_filter

    def per_on(self):
        return self.per_alpha != 0

    def nstep_on(self):
        return self.n_step > 1

    # ---- the rule table: every refusal of a mode or of a combination of modes, stated once
    def _rules(self, grad_hook=None, overlap_collect=False, population=None):
        """(refused, message) row by row, the ranges first; a generator, so a row is evaluated
        only once the rows before it have passed."""
        yield (not isinstance(self.n_step, int) or not 1 <= self.n_step <= NSTEP_MAX,
               f"n_step must be an int in 1 .. {NSTEP_MAX} (1 = multi-step returns off)")
        yield (self.per_alpha < 0 or self.per_alpha != self.per_alpha,
               "per_alpha must be >= 0 (0 = prioritised replay off)")
        # (mode, on, its verbs, its clash with the demonstrations: for PER a bare filter too)
        modes = (("multi-step returns (n_step > 1)", self.nstep_on(), "are", "do",
                  self.demo_fraction != 0 or self.bc_weight != 0),
                 ("prioritised replay (per_alpha > 0)", self.per_on(), "is", "does", self.bc_on()))
        for name, on, be, _, _ in modes[::-1]:
            yield population and on, f"{name} {be} not available to population members"
        yield (population == "batched" and self.bc_q_filter, 'bc_q_filter is not available with '
               'learner="batched" (no population form of the Q-filtered actor kernel)')
        for name, on, _, do, demos in modes:
            yield on and demos, f"{name} {do} not combine with demo_fraction / bc_weight"
            yield (on and grad_hook is not None,
                   f"{name} {do} not combine with a grad_hook (shared policy)")
            yield on and overlap_collect, f"{name} {do} not combine with overlap_collect"

    def check(self, grad_hook=None, overlap_collect=False, population=None, member=None):
        """ValueError for a mode field out of range or a combination that is not built: the rule
        table, then b_demo()'s rules. grad_hook / overlap_collect: what the learner or trainer
        runs with; population: None or PopulationTrainer's learner= ("members", "batched"), with
        `member` the index the message names. Needs no device and no library."""
        for refused, text in self._rules(grad_hook, overlap_collect, population):
            if refused:
                raise ValueError(text if member is None else f"{text}: member {member}")
        try:
            self.b_demo()
        except ValueError as e:
            if member is None:
                raise
            raise ValueError(f"member {member}: {e}") from None

    def b_demo(self):
        """Demonstration rows per batch, round(demo_fraction * batch_size); ValueError for a
        demo_fraction outside [0, 1], a bc_weight without such rows, or bc_q_filter without the
        BC term it filters (needs no device)."""
        n = int(round(self.demo_fraction * self.batch_size))
        if not 0 <= n <= self.batch_size:
            raise ValueError("demo_fraction must lie in [0, 1]")
        if self.bc_weight != 0 and n == 0:
            raise ValueError("bc_weight needs demonstration rows in the batch: demo_fraction * "
                             "batch_size rounds to 0")
        if self.bc_q_filter and (n == 0 or self.bc_weight == 0):
            raise ValueError("bc_q_filter filters the BC term: it needs bc_weight != 0 and "
                             "demonstration rows in the batch (demo_fraction * batch_size >= 1)")
        return n

    def check_n_step(self, grad_hook=None):
        """ValueError for an n_step outside 1 .. NAV_NSTEP_MAX, or n_step > 1 with what
        multi-step returns do not combine with (needs no device)."""
        for refused, text in self._rules(grad_hook):  # the table's rows that name n_step
            if refused and "n_step" in text:
                raise ValueError(text)


# the mode fields, listed once: VecTrainer's keywords, a checkpoint's meta, tools/evaluate.py
MODE_FIELDS = ("demo_fraction", "bc_weight", "q_weight", "bc_q_filter", "per_alpha", "per_beta",
               "per_eps", "n_step")


def mode_meta(cfg):
    """A checkpoint meta's mode keys: the demonstration weights always, a later mode's fields
    only while it is on (a run without them writes the keys it wrote before they existed)."""
    per = cfg.per_on()
    on = dict(per_alpha=per, per_beta=per, per_eps=per, n_step=cfg.nstep_on(),
              bc_q_filter=cfg.bc_q_filter)
    return {k: getattr(cfg, k) for k in MODE_FIELDS if on.get(k, True)}


def mode_kwargs(given):
    """TD3Config's mode fields from VecTrainer's keywords or a checkpoint's meta (other keys
    ignored), a missing one at its default; floats and the flag cast, n_step left to check()."""
    d = TD3Config()
    cast = {float: float, bool: bool}
    return {k: cast.get(type(getattr(d, k)), lambda v: v)(given.get(k, getattr(d, k)))
            for k in MODE_FIELDS}
