"""CartPole: the pole on a cart, the world of the discrete FC nets (FCModel / GRUFCModel with ``is_discrete=True``), as a
world that can live in HBM.  The equations are the textbook ones (gym's constants and gym's explicit Euler order); the
ARITHMETIC is this project's own: integers in one fixed-point format, implemented twice with the same
integers coming out.  Parity with gym is not claimed.

  * ``CartPoleEnv``         -- the host twin in Python ints with a gym-like surface (``reset()``, ``step(a)``, a Discrete-like
                               ``action_space`` with ``n = 2``): observations are the (1, 4) float32 row below;
  * ``DeviceCartPolePool``  -- ``n_envs`` worlds in device memory stepped by a2c_cartpole_step (csrc/cartpole.hip): the
                               Runner's device-pool protocol, driven by the int64 actions the softmax sampler wrote.

Format: Q20, unit 2^-20.  State: x, x_dot, theta, theta_dot, four ints.  ``mul(a, b) = (a * b) >> 20`` (a floor), every
constant an integer of the format (round to nearest): G 9.8, FORCE 10, PML = pole mass * half length 0.05, INV_TOTAL 1 / 1.1,
MP_TOTAL 0.1 / 1.1, PML_TOTAL 0.05 / 1.1, FOUR_THIRDS, TAU 0.02, C6 1/6, C24 1/24, C120 1/120, HALF.

One game frame with action a (0 pushes left, 1 pushes right), in this order:
  1. ``++steps; ++ep_steps``;
  2. t2 = mul(th, th); s = th + mul(th, mul(t2, mul(t2, C120) - C6)); c = ONE + mul(t2, mul(t2, C24) - HALF)   (sin, cos);
  3. temp = mul(+-FORCE + mul(PML, mul(mul(thd, thd), s)), INV_TOTAL);
  4. num = mul(G, s) - mul(c, temp); den = (FOUR_THIRDS - mul(MP_TOTAL, mul(c, c))) >> 1   (half length 0.5; den > 0);
  5. thacc = floor_div(num * 2^20, den)   (the one division, a floor for either sign of num);
  6. xacc = temp - mul(PML_TOTAL, mul(thacc, c));
  7. x += mul(TAU, xd); xd = clamp(xd + mul(TAU, xacc), +-VMAX); th += mul(TAU, thd); thd = clamp(thd + mul(TAU, thacc), +-VMAX)
     with VMAX = 8 (every right-hand side reads the values from before the frame: gym's Euler order);
  8. the reward is 1; over = |x| > X_LIMIT (2.4) or |th| > TH_LIMIT (12 degrees) or ep_steps >= max_episode_steps.
A new episode takes four draws, x, x_dot, theta, theta_dot in this order: each ``d % (2 L + 1) - L``, L = floor(0.05 * 2^20).
Real dones only.

The agent step is that of the Pong worlds (``worlds.HostWorld.advance``; DESIGN.md sections 6g and 6i): ``frame_skip`` ..
``frame_skip_max`` game frames with one action, the k-draw first, then one sticky draw per frame.  ``episodic_life`` /
``clip_rewards`` are keys of the Breakout worlds.

Observation, 4 floats: the state ints times 2^-20, each exact in fp32 (|q| < 2^24) and identical on both sides.

``train()``, env_type "CartPole-device" / "CartPole-host" ("CartPole-v1" stays gym's; the record is ``FAMILY`` below): keys
``max_episode_steps`` (500) and ``frame_skip`` / ``frame_skip_max`` / ``sticky_num`` / ``sticky_den`` as on the Pong worlds;
``prep_fxn="null_prep"``, 2 actions, ``action_shift`` 0 unless given, ``model`` FCModel / GRUFCModel with ``is_discrete=True``
only.  "CartPole-host" steps ``CartPoleEnv``s behind the usual pools (the process pool carries their fp32 frames);
evaluation on host ``CartPoleEnv``s."""
import numpy as np

from . import worlds
from .worlds import DeviceLaneWorldPool, LaneHostWorld, _clamp, check_repeat

N_ACTIONS = 2
FRAC = 20
ONE = 1 << FRAC
UNIT = 2.0 ** -FRAC
CARTPOLE_WORDS, OBS = 12, 4
MAX_EPISODE_STEPS = 1 << 24


def _q(v):
    """a constant as an integer of the format: round to nearest"""
    return int(round(v * ONE))


G, FORCE, PML, INV_TOTAL, MP_TOTAL, PML_TOTAL = _q(9.8), 10 * ONE, _q(0.05), _q(1 / 1.1), _q(0.1 / 1.1), _q(0.05 / 1.1)
FOUR_THIRDS, TAU, HALF, C6, C24, C120 = _q(4 / 3), _q(0.02), ONE // 2, _q(1 / 6), _q(1 / 24), _q(1 / 120)
VMAX = 8 * ONE
X_LIMIT = 2516582                    # floor(2.4 * 2^20)
TH_LIMIT = 219613                    # floor(12 * 2 pi / 360 * 2^20)
RESET_L = 52428                      # floor(0.05 * 2^20)


def mul(a, b):
    """the product of two numbers of the format, floored"""
    return (a * b) >> FRAC


def floor_div(n, d):
    """floor(n / d) for d > 0 the way C has to write it: the truncating quotient, one less where a remainder is left below
    zero (csrc/cartpole_game.h: cartpole_floor_div)"""
    q = abs(n) // d
    if n < 0:
        q = -q
    return q - 1 if n - q * d < 0 else q


def physics(x, xd, th, thd, a):
    """one Euler step of the four state ints with action a (0 left, 1 right) -> the new four"""
    t2 = mul(th, th)
    s = th + mul(th, mul(t2, mul(t2, C120) - C6))
    c = ONE + mul(t2, mul(t2, C24) - HALF)
    temp = mul((FORCE if a else -FORCE) + mul(PML, mul(mul(thd, thd), s)), INV_TOTAL)
    num = mul(G, s) - mul(c, temp)
    den = (FOUR_THIRDS - mul(MP_TOTAL, mul(c, c))) >> 1
    thacc = floor_div(num * ONE, den)
    xacc = temp - mul(PML_TOTAL, mul(thacc, c))
    return (x + mul(TAU, xd), _clamp(xd + mul(TAU, xacc), -VMAX, VMAX), th + mul(TAU, thd),
            _clamp(thd + mul(TAU, thacc), -VMAX, VMAX))


def check_world(max_episode_steps=500, frame_skip=1, sticky_num=0, sticky_den=1, frame_skip_max=None):
    """the bounds a2c_cartpole_reset / a2c_cartpole_step enforce (A2C_ERR_ARG): same ones for the host twin"""
    m = int(max_episode_steps)
    check_repeat(frame_skip, sticky_num, sticky_den, "CartPole", frame_skip_max)
    if not 1 <= m <= MAX_EPISODE_STEPS:
        raise ValueError(f"CartPole: unsupported world max_episode_steps={m} (1 <= max_episode_steps <= {MAX_EPISODE_STEPS})")
    return (m,)


class _Discrete:
    """Discrete-like: ``n`` (SequentialEnvironment reads a discrete env from that)"""
    n = N_ACTIONS


class CartPoleEnv(LaneHostWorld):
    """One CartPole world on the host.  ``reset()`` -> the (1, 4) float32 observation; ``step(a)`` -> (observation, reward,
    done, info), ``a`` an int (the caller has added its ``action_shift``), taken mod 2.  Like a gym env it does not reset
    itself.  ``events`` counts the episode ends by cause, ``x_limit`` / ``theta_limit`` / ``step_limit`` (the first that holds,
    in this order), and ``episode_end`` (with frame skip or sticky actions also ``cut`` and ``sticky``, as the Pong twin) for
    tests that must see every rule at work.  ``truncated`` / ``final_obs``: ``worlds.LaneHostWorld``."""
    WHAT, N_ACTIONS = "CartPole", N_ACTIONS
    action_space = _Discrete()

    def __init__(self, seed=0, env_id=0, max_episode_steps=500, frame_skip=1, sticky_num=0, sticky_den=1, frame_skip_max=None):
        (self.max_episode_steps,) = check_world(max_episode_steps)
        super().__init__(seed, env_id, frame_skip, sticky_num, sticky_den, ("x_limit", "theta_limit", "step_limit", "episode_end"),
                         frame_skip_max)
        self.x = self.xd = self.th = self.thd = 0

    def new_episode(self):
        """the reset without its observation"""
        self.x, self.xd, self.th, self.thd = (self._draw() % (2 * RESET_L + 1) - RESET_L for _ in range(4))
        self.ep_steps = self.prev = 0
        self.over = False

    def _frame(self, a):
        """one game frame with action ``a`` (0 left, 1 right) -> (reward, done)"""
        self.steps += 1
        self.ep_steps += 1
        self.x, self.xd, self.th, self.thd = physics(self.x, self.xd, self.th, self.thd, a)
        cause = ("x_limit" if abs(self.x) > X_LIMIT else "theta_limit" if abs(self.th) > TH_LIMIT else
                 "step_limit" if self.ep_steps >= self.max_episode_steps else None)
        if cause is not None:
            self.over = True
            self.limit_alone = cause == "step_limit"
            self.events[cause] += 1
            self.events["episode_end"] += 1
        return 1.0, cause is not None

    def obs(self):
        """the (1, 4) float32 observation: int -> fp32 first (exact), then one exact multiply by 2^-20"""
        return (np.array([self.x, self.xd, self.th, self.thd], dtype=np.float32) * np.float32(UNIT))[None]

    render_rgb = obs


class DeviceCartPolePool(DeviceLaneWorldPool):
    """``n_envs`` CartPole worlds in device memory (the Runner's device-pool protocol).  Env j is the world ``CartPoleEnv(seed,
    env_id=env_id0 + j, ...)``: same draws, same observations.  ``step`` / ``device_step`` take the address of env 0's int64
    action and the element stride between envs.  done == reset: real dones only."""
    WHAT = "CartPole"
    frame_shape = (1, OBS)

    def __init__(self, n_envs, device="cuda", seed=0, max_episode_steps=500, env_id0=0, frame_skip=1, sticky_num=0,
                 sticky_den=1, frame_skip_max=None):
        super().__init__(n_envs, device, seed, env_id0, check_world(max_episode_steps), frame_skip, sticky_num, sticky_den,
                         frame_skip_max)


# picklable ``env_fn``: ``CartPoleFactory(env_id=j, **world)()`` is a ``CartPoleEnv``
CartPoleFactory = worlds.factory_of(CartPoleEnv)
FAMILY = worlds.WorldFamily(__name__, "CartPole", check_world, (("max_episode_steps", 500),), "null_prep",
                            rule_keys=("frame_skip_max",), models=worlds.FC_MODELS,
                            takes="one of two int actions on (1, 4) observations")
RULE_KEYS, rules_from_hyps, world_from_hyps = FAMILY.rule_keys, FAMILY.rules_from_hyps, FAMILY.world_from_hyps
