"""Point: a point mass chasing targets, the continuous-control world of the Gaussian nets (FCModel / GRUFCModel with
``is_discrete=False``), as a world that can live in HBM.  The rules are this project's own, integer
arithmetic throughout, implemented twice with the same integers coming out:

  * ``PointEnv``         -- the host twin in Python ints with a gym-like surface (``reset()``, ``step(a)``, a Box-like
                            ``action_space`` of shape (2,)): observations are the (1, 8) float32 row below;
  * ``DevicePointPool``  -- ``n_envs`` worlds in device memory stepped by a2c_point_step (csrc/point.hip): the Runner's
                            device-pool protocol, driven by the FLOAT action rows a2c_gauss_head wrote.

Field: positions 0 .. P - 1 = 4095 per axis.  State: the point (px, py), its velocity (vx, vy), the target (tx, ty), the
targets reached this episode ``got``.  ``place(d) = (512 + (d & 0xFFF) % 3072, 512 + ((d >> 12) & 0xFFF) % 3072)``.  A new
episode takes two draws: the first places the point, the second the target; vx = vy = got = 0.

The action is two floats.  The ONE place where floats enter is the quantiser: per component x = fp32(a + action_shift) (one
rounded add; the Runner's host path adds the shift itself and the twin receives the sum), q = 0 for a NaN, else
rint(clamp(x, -1, 1) * 64) with ties to even: -64 .. 64, +-inf giving +-64.  x * 64 is exact, so NumPy and the device agree
on every q.  The game frames take the pair packed into one int, (qx & 0xFF) | ((qy & 0xFF) << 8) (each byte sign-extended on
the way out): packed 0 is (0, 0), what ``prev = 0`` after an episode end means for sticky actions.

One game frame, in this order:
  1. ``++steps; ++ep_steps``;
  2. d0 = (|px - tx| + |py - ty|) // CELL;
  3. per axis: v = clamp(v + floor(q / 8), -VMAX, VMAX), p += v; p < 0 -> p = 0, v = 0; p > P - 1 -> p = P - 1, v = 0 (wall);
  4. d1 like d0;  5. r = d0 - d1;  6. d1 == 0: r += REACH_BONUS, ``++got``;
  7. over = got >= targets_to_win or ep_steps >= max_episode_steps;
  8. over: a new episode; else a reached target is replaced with one draw.
Real dones only; rewards are small integers (|r| <= 3 without the bonus).

The agent step is that of the Pong worlds (``worlds.HostWorld.advance``; DESIGN.md sections 6g and 6i): ``frame_skip`` ..
``frame_skip_max`` game frames with one action (action repeat), the k-draw first, then one sticky draw per frame before the
frame's own draws.  ``episodic_life`` / ``clip_rewards`` are keys of the Breakout worlds.

Observation, 8 floats, each an integer times a power of two, so exact in fp32 and identical on both sides:
  [(2px - 4095) / 4096, (2py - 4095) / 4096, vx / 64, vy / 64, (tx - px) / 4096, (ty - py) / 4096, got / 8, 1]

``train()``, env_type "Point-device" / "Point-host" (the record is ``FAMILY`` below): keys ``targets_to_win`` (3),
``max_episode_steps`` (1000) and ``frame_skip`` / ``frame_skip_max`` / ``sticky_num`` / ``sticky_den`` as on the Pong worlds;
``prep_fxn="null_prep"``, ``is_discrete=False``, 2 float actions, ``model`` FCModel / GRUFCModel only (anything else is a
ValueError before anything is allocated).  ``DevicePointPool`` reads the float action rows on the device; "Point-host" steps
``PointEnv``s behind ``env_pool`` "serial" (the default) or "process_f32"; evaluation on host ``PointEnv``s."""
import numpy as np

from . import worlds
from .worlds import DeviceLaneWorldPool, LaneHostWorld, _clamp, check_repeat

ACTION_SIZE = 2
P, VMAX, CELL, REACH_BONUS = 4096, 64, 64, 10
Q = 64                                            # the quantiser's scale: q = -Q .. Q, Q / 8 velocity units a frame
POINT_WORDS, OBS = 16, 8
MAX_TARGETS, MAX_EPISODE_STEPS = 8, 1 << 24


def check_world(targets_to_win=3, max_episode_steps=1000, frame_skip=1, sticky_num=0, sticky_den=1, frame_skip_max=None):
    """the bounds a2c_point_reset / a2c_point_step enforce (A2C_ERR_ARG): same ones for the host twin"""
    n, m = int(targets_to_win), int(max_episode_steps)
    check_repeat(frame_skip, sticky_num, sticky_den, "Point", frame_skip_max)
    if not (1 <= n <= MAX_TARGETS and 1 <= m <= MAX_EPISODE_STEPS):
        raise ValueError(f"Point: unsupported world targets_to_win={n} max_episode_steps={m} (1 <= targets_to_win <= "
                         f"{MAX_TARGETS}, 1 <= max_episode_steps <= {MAX_EPISODE_STEPS})")
    return n, m


def quantise(a, shift=0.0):
    """the quantiser in NumPy: float actions (any shape) -> int32 q in -64 .. 64.  x = fp32(a + shift), one rounded add; NaN
    -> 0; else rint(clip(x, -1, 1) * 64), ties to even (the product is exact)"""
    with np.errstate(invalid="ignore"):
        x = np.asarray(a, dtype=np.float32) + np.float32(shift)
        q = np.rint(np.clip(x, np.float32(-1), np.float32(1)) * np.float32(Q))
    return np.where(np.isnan(x), np.float32(0), q).astype(np.int32)


def pack(qx, qy):
    """the pair as the one int a game frame takes; 0 is (0, 0)"""
    return (int(qx) & 0xFF) | ((int(qy) & 0xFF) << 8)


def unpack(a):
    """-> (qx, qy): each byte sign-extended"""
    sx = lambda b: b - 256 if b & 0x80 else b
    return sx(a & 0xFF), sx((a >> 8) & 0xFF)


def place(d):
    return 512 + (d & 0xFFF) % 3072, 512 + ((d >> 12) & 0xFFF) % 3072


class _Box:
    """Box-like: ``shape`` and no ``n`` (SequentialEnvironment reads a continuous env from that)"""
    shape = (ACTION_SIZE,)
    low, high = -1.0, 1.0


class PointEnv(LaneHostWorld):
    """One Point world on the host.  ``reset()`` -> the (1, 8) float32 observation; ``step(a)`` -> (observation, reward,
    done, info), ``a`` two floats (the caller has added its ``action_shift``).  Like a gym env it does not reset itself.
    ``events`` counts wall hits, targets reached and episode ends by targets / by the step cap (with frame skip or sticky
    actions also ``cut`` and ``sticky``, as the Pong twin) for tests that must see every rule at work.  ``truncated`` /
    ``final_obs``: ``worlds.LaneHostWorld``."""
    WHAT = "Point"
    action_space = _Box()

    def __init__(self, seed=0, env_id=0, targets_to_win=3, max_episode_steps=1000, frame_skip=1, sticky_num=0, sticky_den=1,
                 frame_skip_max=None):
        self.targets_to_win, self.max_episode_steps = check_world(targets_to_win, max_episode_steps)
        super().__init__(seed, env_id, frame_skip, sticky_num, sticky_den, ("wall", "reach", "end_targets", "end_cap"),
                         frame_skip_max)
        self.px = self.py = self.tx = self.ty = 512
        self.vx = self.vy = self.got = 0

    def new_episode(self):
        """the reset without its observation"""
        self.px, self.py = place(self._draw())
        self.tx, self.ty = place(self._draw())
        self.vx = self.vy = self.got = self.ep_steps = self.prev = 0
        self.over = False

    def _action(self, action):
        q = quantise(np.asarray(action, dtype=np.float32).reshape(ACTION_SIZE))
        return pack(q[0], q[1])

    def _cells(self):
        return (abs(self.px - self.tx) + abs(self.py - self.ty)) // CELL

    def _axis(self, p, v, q):
        v = _clamp(v + (q >> 3), -VMAX, VMAX)           # q >> 3 = floor(q / 8)
        p += v
        if p < 0:
            p, v = 0, 0
            self.events["wall"] += 1
        elif p > P - 1:
            p, v = P - 1, 0
            self.events["wall"] += 1
        return p, v

    def _frame(self, a):
        """one game frame with the packed pair ``a`` -> (reward, done)"""
        qx, qy = unpack(a)
        self.steps += 1
        self.ep_steps += 1
        d0 = self._cells()
        self.px, self.vx = self._axis(self.px, self.vx, qx)
        self.py, self.vy = self._axis(self.py, self.vy, qy)
        d1 = self._cells()
        rew = d0 - d1
        if d1 == 0:
            rew += REACH_BONUS
            self.got += 1
            self.events["reach"] += 1
        done = self.got >= self.targets_to_win or self.ep_steps >= self.max_episode_steps
        if done:
            self.over = True
            self.limit_alone = self.got < self.targets_to_win
            self.events["end_targets" if self.got >= self.targets_to_win else "end_cap"] += 1
        elif d1 == 0:
            self.tx, self.ty = place(self._draw())
        return float(rew), done

    def obs(self):
        """the (1, 8) float32 observation"""
        o = np.array([(2 * self.px - (P - 1)) / 4096, (2 * self.py - (P - 1)) / 4096, self.vx / 64, self.vy / 64,
                      (self.tx - self.px) / 4096, (self.ty - self.py) / 4096, self.got / 8, 1.0], dtype=np.float32)
        return o[None]

    render_rgb = obs


class DevicePointPool(DeviceLaneWorldPool):
    """``n_envs`` Point worlds in device memory (the Runner's device-pool protocol).  Env j is the world ``PointEnv(seed,
    env_id=env_id0 + j, ...)``: same draws, same observations.  ``float_actions``: ``step`` / ``device_step`` take the address
    of env 0's two float32 actions and the stride between envs IN FLOATS (a row of a continuous rollout buffer), and
    ``action_shift`` is a float.  done == reset: real dones only."""
    WHAT = "Point"
    frame_shape = (1, OBS)
    float_actions = True
    n_act = ACTION_SIZE

    def __init__(self, n_envs, device="cuda", seed=0, targets_to_win=3, max_episode_steps=1000, env_id0=0, frame_skip=1,
                 sticky_num=0, sticky_den=1, frame_skip_max=None):
        super().__init__(n_envs, device, seed, env_id0, check_world(targets_to_win, max_episode_steps), frame_skip, sticky_num,
                         sticky_den, frame_skip_max)


# picklable ``env_fn``: ``PointFactory(env_id=j, **world)()`` is a ``PointEnv``
PointFactory = worlds.factory_of(PointEnv)
FAMILY = worlds.WorldFamily(__name__, "Point", check_world, (("targets_to_win", 3), ("max_episode_steps", 1000)), "null_prep",
                            rule_keys=("frame_skip_max",), models=worlds.FC_MODELS)
RULE_KEYS, rules_from_hyps, world_from_hyps = FAMILY.rule_keys, FAMILY.rules_from_hyps, FAMILY.world_from_hyps
