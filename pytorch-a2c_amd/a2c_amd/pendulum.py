"""Pendulum: the pendulum swing-up, the textbook continuous-control world of the Gaussian nets (FCModel / GRUFCModel with
``is_discrete=False``), as a world that can live in HBM.  The equations are the textbook ones (gym's ``Pendulum-v1``: its
constants and its Euler order); the ARITHMETIC is this project's own: integers in one fixed-point
format, implemented twice with the same integers coming out.  Parity with gym is not claimed.

  * ``PendulumEnv``         -- the host twin in Python ints with a gym-like surface (``reset()``, ``step(a)``, a Box-like
                               ``action_space`` of shape (1,)): observations are the (1, 4) float32 row below;
  * ``DevicePendulumPool``  -- ``n_envs`` worlds in device memory stepped by a2c_pendulum_step (csrc/pendulum.hip): the
                               Runner's device-pool protocol, driven by the FLOAT action a2c_gauss_head wrote for each env.

Format: Q20, unit 2^-20.  State: th in [-PI, PI) (0 is upright) and thd in [-VMAX, VMAX], two ints.  ``mul(a, b) = (a * b)
>> 20`` (a floor); there is no division.  Constants, integers of the format rounded to nearest: PI, TWO_PI = 2 PI, HALF_PI,
C075 0.75 (= 3 g / (2 l) dt), C015 0.15 (= 3 / (m l^2) dt), DT 0.05, C01 0.1, C0001 0.001, VMAX 8, ONE.

The action is one float.  The ONE place where floats enter is the quantiser: x = fp32(a + action_shift) (one rounded add; the
Runner's host path adds the shift itself and the twin receives the sum), q = 0 for a NaN, else rint(clamp(x, -2, 2) * 32) with
ties to even: -64 .. 64, +-inf giving +-64.  x * 32 is exact, so NumPy and the device agree on every q.  The game frames take
q itself as their int; the torque is u = q << 15, q / 32 in Q20.  ``prev = 0`` after an episode end is zero torque.

``sincos(th)``: reflected to |x| <= HALF_PI (x = +-PI - th outside, the cosine negated there); x2 = mul(x, x);
  p = ONE; for k in (110, 72, 42, 20, 6): p = ONE - mul(mul(x2, q(1/k)), p); sin = mul(x, p);
  p = ONE; for k in (132, 90, 56, 30, 12, 2): p = ONE - mul(mul(x2, q(1/k)), p); cos = +-p.

One game frame with the quantised action q, in this order (gym's):
  1. ``++steps; ++ep_steps``;
  2. cost = mul(th, th) + mul(C01, mul(thd, thd)) + mul(C0001, mul(u, u)), from the values before the frame;
  3. thd = clamp(thd + mul(C075, sin th) + mul(C015, u), +-VMAX);
  4. th += mul(DT, thd) with the new thd, then one wrap by TWO_PI into [-PI, PI);
  5. over = ep_steps >= max_episode_steps: only the step cap ends an episode.  Real dones only.
A new episode takes two draws: th = d % TWO_PI - PI, then thd = d % (2 ONE + 1) - ONE.

Reward: the frame's reward is the int -(cost >> 12) in units of 2^-8, -4166 .. 0.  What the agent sees is that int times 2^-8
as fp32, exact, also summed over the 8 frames of an agent step.  The device's episode counters are whole reward units:
every closed episode's sum FLOORED (-833.6 -> -834), so ``DevicePendulumPool.episode_stats()`` and the reward average the
Runner publishes from it lie less than one unit below what host twins give.

The agent step is that of the Pong worlds (``worlds.HostWorld.advance``; DESIGN.md sections 6g and 6i): ``frame_skip`` ..
``frame_skip_max`` game frames with one action, the k-draw first, then one sticky draw per frame.  ``episodic_life`` /
``clip_rewards`` are keys of the Breakout worlds.

Observation, 4 floats: (cos th, sin th, thd) times 2^-20 and a 0 (the post form moves planes as 16-byte quads), each exact in
fp32 (|int| <= 2^23) and identical on both sides.

``train()``, env_type "Pendulum-device" / "Pendulum-host" ("Pendulum-v1" stays gym's; the record is ``FAMILY`` below): keys
``max_episode_steps`` (200, at most 2^16) and ``frame_skip`` / ``frame_skip_max`` / ``sticky_num`` / ``sticky_den`` as on the
Pong worlds; ``prep_fxn="null_prep"``, ``is_discrete=False``, 1 float action (the torque, clamped to +-2), and the refusals
and pools of the Point worlds: ``model`` FCModel / GRUFCModel only, "Pendulum-host" behind ``env_pool`` "serial" (the default)
or "process_f32"; evaluation on host ``PendulumEnv``s."""
import numpy as np

from . import worlds
from .worlds import DeviceLaneWorldPool, LaneHostWorld, _clamp, check_repeat

ACTION_SIZE = 1
FRAC = 20
ONE = 1 << FRAC
UNIT = 2.0 ** -FRAC
PENDULUM_WORDS, OBS = 12, 4
MAX_EPISODE_STEPS = 1 << 16
Q, Q_SHIFT, MAX_TORQUE = 32, 15, 2.0            # the quantiser's scale: q = -64 .. 64, the torque q / 32 = q << 15 in Q20
REW_SHIFT, REW_FRAC = 12, 8                      # reward int = -(cost >> 12), units of 2^-8
REW_UNIT = 2.0 ** -REW_FRAC


def _q(v):
    """a constant as an integer of the format: round to nearest"""
    return int(round(v * ONE))


PI, HALF_PI = 3294199, 1647099
TWO_PI = 2 * PI
C075, C015, DT, C01, C0001 = 786432, 157286, 52429, 104858, 1049
VMAX = 8 * ONE
SIN_K, COS_K = (110, 72, 42, 20, 6), (132, 90, 56, 30, 12, 2)
SIN_R, COS_R = tuple(_q(1 / k) for k in SIN_K), tuple(_q(1 / k) for k in COS_K)


def mul(a, b):
    """the product of two numbers of the format, floored"""
    return (a * b) >> FRAC


def sincos(th):
    """(sin, cos) of th in [-PI, PI) as integers of the format"""
    out = th > HALF_PI or th < -HALF_PI
    x = ((PI if th > 0 else -PI) - th) if out else th
    x2 = mul(x, x)
    p = ONE
    for r in SIN_R:
        p = ONE - mul(mul(x2, r), p)
    s = mul(x, p)
    p = ONE
    for r in COS_R:
        p = ONE - mul(mul(x2, r), p)
    return s, (-p if out else p)


def physics(th, thd, q):
    """one Euler step of the two state ints with the quantised action q -> (th, thd, cost, clamped, wrap): the new two, the
    cost of the frame in Q20 (from the old two), whether the speed clamp held, and the wrap taken (+1: th left [-PI, PI) at
    PI and TWO_PI was taken off, -1: the other side, 0: none)"""
    u = q << Q_SHIFT
    cost = mul(th, th) + mul(C01, mul(thd, thd)) + mul(C0001, mul(u, u))
    s, _ = sincos(th)
    raw = thd + mul(C075, s) + mul(C015, u)
    nthd = _clamp(raw, -VMAX, VMAX)
    nth = th + mul(DT, nthd)
    wrap = 0
    if nth >= PI:
        nth, wrap = nth - TWO_PI, 1
    elif nth < -PI:
        nth, wrap = nth + TWO_PI, -1
    return nth, nthd, cost, raw != nthd, wrap


def check_world(max_episode_steps=200, frame_skip=1, sticky_num=0, sticky_den=1, frame_skip_max=None):
    """the bounds a2c_pendulum_reset / a2c_pendulum_step enforce (A2C_ERR_ARG): same ones for the host twin"""
    m = int(max_episode_steps)
    check_repeat(frame_skip, sticky_num, sticky_den, "Pendulum", frame_skip_max)
    if not 1 <= m <= MAX_EPISODE_STEPS:
        raise ValueError(f"Pendulum: unsupported world max_episode_steps={m} (1 <= max_episode_steps <= {MAX_EPISODE_STEPS})")
    return (m,)


def quantise(a, shift=0.0):
    """the quantiser in NumPy: float actions (any shape) -> int32 q in -64 .. 64.  x = fp32(a + shift), one rounded add; NaN
    -> 0; else rint(clip(x, -2, 2) * 32), ties to even (the product is exact)"""
    with np.errstate(invalid="ignore"):
        x = np.asarray(a, dtype=np.float32) + np.float32(shift)
        q = np.rint(np.clip(x, np.float32(-MAX_TORQUE), np.float32(MAX_TORQUE)) * np.float32(Q))
    return np.where(np.isnan(x), np.float32(0), q).astype(np.int32)


class _Box:
    """Box-like: ``shape`` and no ``n`` (SequentialEnvironment reads a continuous env from that)"""
    shape = (ACTION_SIZE,)
    low, high = -MAX_TORQUE, MAX_TORQUE


class PendulumEnv(LaneHostWorld):
    """One Pendulum world on the host.  ``reset()`` -> the (1, 4) float32 observation; ``step(a)`` -> (observation, reward,
    done, info), ``a`` one float (the caller has added its ``action_shift``).  Like a gym env it does not reset itself.
    ``events`` counts the wraps of th by side (``wrap_pos``: past PI), the frames whose speed was clamped and the episode ends
    (``end_cap``: the only kind; with frame skip or sticky actions also ``cut`` and ``sticky``, as the Pong twin) for tests
    that must see every rule at work.  ``truncated`` / ``final_obs``: ``worlds.LaneHostWorld`` (every end is truncated)."""
    WHAT = "Pendulum"
    action_space = _Box()

    def __init__(self, seed=0, env_id=0, max_episode_steps=200, frame_skip=1, sticky_num=0, sticky_den=1, frame_skip_max=None):
        (self.max_episode_steps,) = check_world(max_episode_steps)
        super().__init__(seed, env_id, frame_skip, sticky_num, sticky_den, ("wrap_pos", "wrap_neg", "clamp", "end_cap"),
                         frame_skip_max)
        self.th = self.thd = 0

    def new_episode(self):
        """the reset without its observation"""
        self.th = self._draw() % TWO_PI - PI
        self.thd = self._draw() % (2 * ONE + 1) - ONE
        self.ep_steps = self.prev = 0
        self.over = False

    def _action(self, action):
        return int(quantise(np.asarray(action, dtype=np.float32).reshape(ACTION_SIZE))[0])

    def _frame(self, q):
        """one game frame with the quantised action ``q`` -> (reward, done); the reward is an int times 2^-8"""
        self.steps += 1
        self.ep_steps += 1
        self.th, self.thd, cost, clamped, wrap = physics(self.th, self.thd, q)
        self.events["clamp"] += clamped
        if wrap:
            self.events["wrap_pos" if wrap > 0 else "wrap_neg"] += 1
        done = self.ep_steps >= self.max_episode_steps
        if done:
            self.over = True
            self.limit_alone = True
            self.events["end_cap"] += 1
        return -(cost >> REW_SHIFT) * REW_UNIT, done

    def obs(self):
        """the (1, 4) float32 observation: int -> fp32 first (exact), then one exact multiply by 2^-20"""
        s, c = sincos(self.th)
        return (np.array([c, s, self.thd, 0], dtype=np.float32) * np.float32(UNIT))[None]

    render_rgb = obs


class DevicePendulumPool(DeviceLaneWorldPool):
    """``n_envs`` Pendulum worlds in device memory (the Runner's device-pool protocol).  Env j is the world ``PendulumEnv(seed,
    env_id=env_id0 + j, ...)``: same draws, same observations.  ``float_actions``: ``step`` / ``device_step`` take the address
    of env 0's ONE float32 action and the stride between envs IN FLOATS (a row of a continuous rollout buffer: >= 1), and
    ``action_shift`` is a float.  done == reset: real dones only.  ``episode_stats()`` is whole reward units: the sum of
    every closed episode's reward floored."""
    WHAT = "Pendulum"
    frame_shape = (1, OBS)
    float_actions = True
    n_act = ACTION_SIZE

    def __init__(self, n_envs, device="cuda", seed=0, max_episode_steps=200, env_id0=0, frame_skip=1, sticky_num=0,
                 sticky_den=1, frame_skip_max=None):
        super().__init__(n_envs, device, seed, env_id0, check_world(max_episode_steps), frame_skip, sticky_num, sticky_den,
                         frame_skip_max)


# picklable ``env_fn``: ``PendulumFactory(env_id=j, **world)()`` is a ``PendulumEnv``
PendulumFactory = worlds.factory_of(PendulumEnv)
FAMILY = worlds.WorldFamily(__name__, "Pendulum", check_world, (("max_episode_steps", 200),), "null_prep",
                            rule_keys=("frame_skip_max",), models=worlds.FC_MODELS)
RULE_KEYS, rules_from_hyps, world_from_hyps = FAMILY.rule_keys, FAMILY.rules_from_hyps, FAMILY.world_from_hyps
