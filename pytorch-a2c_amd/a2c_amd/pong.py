"""Pong: the reference's main env (``pong_prep``, the "Pong" done override, ``action_shift``), as a world that can live
in HBM.  The rules are this project's own (parity with ALE is not claimed), integer arithmetic
throughout, implemented twice with the same integers coming out:

  * ``PongEnv``         -- the host twin in NumPy / Python ints with a gym-like surface (``reset()``, ``step(a)``,
                           ``action_space.n == 3``): RAW 210 x 160 x 3 uint8 frames in ALE's layout, which the reference's
                           ``pong_prep`` turns into the 80 x 80 binary frame ``prepped()`` returns directly;
  * ``DevicePongPool``  -- ``n_envs`` worlds in device memory stepped by a2c_pong_step (csrc/pong.hip): the Runner's
                           device-pool protocol, driven by the actions the sampler wrote.  Frames arrive prepped.

Field: 80 x 80 pixels, (x, y) = (column, row), objects named by their top-left pixel.  Opponent paddle: columns 8..9,
agent paddle: columns 70..71, both 2 x 8, rows y..y+7 with 0 <= y <= 72.  Ball: 2 x 2, 0 <= y <= 78.

One step, in this order (every division below is between non-negative ints):
  1. the agent takes ``a = (action + action_shift) mod 3`` (0 stay, 1 up, 2 down): its paddle moves 2 pixels, clamped;
  2. one draw ``d``; if ``d mod opp_skill_den < opp_skill_num`` the opponent moves 1 pixel towards the ball's centre
     (compares ball y + 1 with paddle y + 4; the ball's position BEFORE it moves), clamped;
  3. the ball moves by (vx, vy); y < 0 -> y = -y, y > 78 -> y = 156 - y, vy = -vy each time (wall bounce);
  4. paddle hit: the ball reaches a paddle's face in this step (agent: vx > 0, old x + 1 < 70 <= new x + 1; opponent:
     vx < 0, old x > 9 >= new x) and overlaps its rows (ball y + 1 >= paddle y and ball y <= paddle y + 7): the ball
     rests against the face (x = 68 / x = 10), ``off = ball y + 1 - paddle y`` (0..8) sets vy = HIT_VY[off] and
     |vx| = HIT_SPEED[off], vx pointing away from the paddle;
  5. point: new x >= 72 (the agent missed: reward -1) or new x <= 6 (the opponent missed: reward +1);
  6. the episode ends (the REAL done) when a score reaches ``points_to_win`` or after ``max_episode_steps`` steps;
     otherwise, after a point, the ball is served: one draw ``d``, ball at (39, 39), vy = (d >> 1) mod 5 - 2, |vx| = 1
     towards the side that lost the point.
A reset zeroes scores and the episode-step counter, centres both paddles (y = 36) and serves with one draw: direction
from ``d & 1`` (1: towards the agent), vy as above.  Randomness is counter based: draw i of env e is
``hash32(seed, e, i)``, the mixing function of the Snake worlds.

Frame skip and sticky actions (``frame_skip`` 1..8, ``sticky_num`` / ``sticky_den`` with the bounds of
``opp_skill_*``): the step above is one GAME FRAME, and one AGENT step -- ``step(a)`` / ``advance(a)``, one launch of
a2c_pong_step_skip -- is ``frame_skip`` of them with the same requested action ``a``.  Game frame s = 0 .. k-1: x = a; when
``sticky_num > 0`` one draw ``d`` is taken BEFORE the frame's own draws and x = ``prev`` (the action the previous game frame
executed) if ``d mod sticky_den < sticky_num``; prev = x; the frame runs with x and its reward is added to the agent
step's.  A frame that ends the episode zeroes ``prev`` and the remaining frames are DROPPED (``events["cut"]``).  The
agent step's done is the real done; the "Pong" done is that or a non-zero summed reward.  At most one point falls in an
agent step (after a serve the ball needs at least 33 frames to reach a goal line, and k <= 8).  ``steps``, ``ep_steps`` and
``max_episode_steps`` count game frames.  With ``sticky_num == 0`` no draw is taken and ``prev`` stays 0: k = 1 is the world
above word for word, k > 1 is that world stepped k times with one action and cut at the real done.

Random frame skip (a2c_pong_step_rules): with ``frame_skip_max`` (``frame_skip`` .. 8; None =
``frame_skip``) above ``frame_skip`` the agent step first takes ONE draw ``d``, before its first sticky draw, and plays
k = frame_skip + d mod (frame_skip_max - frame_skip + 1) game frames: ``frame_skip=2, frame_skip_max=4, sticky_num=1,
sticky_den=4`` is the stepping rule of ``Pong-v0``.  Episodic life and reward clipping are keys of the Breakout worlds: here
a point closes every step already and |reward| <= 1.

``train()``, env_type "Pong-device" / "Pong-host" (the record is ``FAMILY`` below): keys ``points_to_win`` (21),
``max_episode_steps`` (10000), ``opp_skill_num`` / ``opp_skill_den`` (3 / 4), ``frame_skip``, ``sticky_num``, ``sticky_den``
and ``frame_skip_max``, for the training pool and the evaluation worlds alike; ``episodic_life`` / ``clip_rewards`` are a
ValueError.  ``prep_fxn="pong_prep"`` (the process pool carries the {0, 1} frames packed, one bit per pixel), 3 actions,
``action_shift`` 0 unless given, the "Pong" done override applies; evaluation on host ``PongEnv``s."""
import numpy as np

from . import worlds
from .worlds import (MAX_FRAME_SKIP, MAX_STICKY_DEN, _M, DeviceRegisterWorldPool, HostWorld, _clamp, _env_id0,  # noqa: F401
                     check_repeat, check_rules, hash32, repeat_from_hyps)

N_ACTIONS = 3
W = H = 80
PADDLE_H, PADDLE_W, BALL = 8, 2, 2
OPP_X, AGENT_X = 8, 70
PADDLE_MAX_Y, BALL_MAX_Y = H - PADDLE_H, H - BALL
PADDLE_START_Y, SERVE_X, SERVE_Y = 36, 39, 39
AGENT_SPEED, OPP_SPEED = 2, 1
HIT_VY = (-2, -2, -1, -1, 0, 1, 1, 2, 2)         # by off = ball y + 1 - paddle y
HIT_SPEED = (2, 2, 1, 1, 1, 1, 1, 2, 2)          # |vx| after the hit
MISS_RIGHT, MISS_LEFT = AGENT_X + PADDLE_W, OPP_X - BALL      # ball x >= 72: agent missed; ball x <= 6: opponent missed
MAX_POINTS, MAX_EPISODE_STEPS, MAX_SKILL_DEN = 21, 1 << 24, 1 << 16
# raw frames (ALE's layout): the playfield is rows 35..194 at 2 x scale; channel 0 of the two background colours is what
# pong_prep removes
RAW_H, RAW_W, RAW_TOP = 210, 160, 35
FIELD_BG, BORDER_BG = (144, 72, 17), (109, 118, 43)
OPP_RGB, AGENT_RGB, BALL_RGB = (213, 130, 74), (92, 186, 92), (236, 236, 236)


def check_world(points_to_win=21, max_episode_steps=10000, opp_skill_num=3, opp_skill_den=4, frame_skip=1, sticky_num=0,
                sticky_den=1, frame_skip_max=None):
    """the bounds a2c_pong_step / a2c_pong_step_skip / a2c_pong_step_rules enforce (A2C_ERR_ARG): same ones for the host twin"""
    p, m, n, d = int(points_to_win), int(max_episode_steps), int(opp_skill_num), int(opp_skill_den)
    check_repeat(frame_skip, sticky_num, sticky_den, frame_skip_max=frame_skip_max)
    if not (1 <= p <= MAX_POINTS and 1 <= m <= MAX_EPISODE_STEPS and 1 <= d <= MAX_SKILL_DEN and 0 <= n <= d):
        raise ValueError(f"Pong: unsupported world points_to_win={p} max_episode_steps={m} opp_skill={n}/{d} (1 <= "
                         f"points_to_win <= {MAX_POINTS}, 1 <= max_episode_steps <= {MAX_EPISODE_STEPS}, 1 <= opp_skill_den "
                         f"<= {MAX_SKILL_DEN}, 0 <= opp_skill_num <= opp_skill_den)")
    return p, m, n, d


class _ActionSpace:
    n = N_ACTIONS


class PongEnv(HostWorld):
    """One Pong world on the host.  ``reset()`` -> raw (210, 160, 3) uint8 frame; ``step(a)`` -> (frame, reward, done,
    info) with the REAL done (a score at ``points_to_win``, or the step limit).  Like a gym env it does not reset itself:
    the caller does -- the Runner does, which yields exactly what the device world returns.  ``events`` counts what
    happened (wall bounces, paddle hits, points, episode ends; with frame skip or sticky actions also ``cut``: episode ends
    that dropped game frames of their agent step, and ``sticky``: game frames that kept an action other than the requested one) for tests that must see every
    rule at work.  ``step`` / ``advance`` are the AGENT step: ``frame_skip`` game frames (module docstring)."""
    WHAT, N_ACTIONS = "Pong", N_ACTIONS
    action_space = _ActionSpace()

    def __init__(self, seed=0, env_id=0, points_to_win=21, max_episode_steps=10000, opp_skill_num=3, opp_skill_den=4,
                 frame_skip=1, sticky_num=0, sticky_den=1, frame_skip_max=None):
        self.points_to_win, self.max_episode_steps, self.skill_num, self.skill_den = check_world(
            points_to_win, max_episode_steps, opp_skill_num, opp_skill_den)
        super().__init__(seed, env_id, frame_skip, sticky_num, sticky_den,
                         ("wall", "hit_agent", "hit_opp", "agent_point", "opp_point", "episode_end"), frame_skip_max)
        self.agent_y = self.opp_y = PADDLE_START_Y
        self.ball_x, self.ball_y, self.vx, self.vy = SERVE_X, SERVE_Y, 1, 0
        self.score_agent = self.score_opp = 0

    def _serve(self, d, towards_agent):
        self.ball_x, self.ball_y = SERVE_X, SERVE_Y
        self.vx, self.vy = (1 if towards_agent else -1), (d >> 1) % 5 - 2

    def new_episode(self):
        """the reset without its frame"""
        self.agent_y = self.opp_y = PADDLE_START_Y
        self.score_agent = self.score_opp = self.ep_steps = self.prev = 0
        d = self._draw()
        self._serve(d, bool(d & 1))
        self.over = False

    def _check_step(self, total):
        assert abs(total) <= 1, "more than one point in one agent step"

    def _frame(self, a):
        """one game frame with action ``a`` in 0..2 -> (reward, done)"""
        self.steps += 1
        self.ep_steps += 1
        # 1. the agent's paddle
        self.agent_y = _clamp(self.agent_y + (-AGENT_SPEED if a == 1 else (AGENT_SPEED if a == 2 else 0)), 0, PADDLE_MAX_Y)
        # 2. the opponent's paddle: towards the ball's centre, on the steps the draw allows
        if self._draw() % self.skill_den < self.skill_num:
            c_ball, c_pad = self.ball_y + 1, self.opp_y + PADDLE_H // 2
            self.opp_y = _clamp(self.opp_y + (-OPP_SPEED if c_ball < c_pad else (OPP_SPEED if c_ball > c_pad else 0)),
                                0, PADDLE_MAX_Y)
        # 3. the ball, the walls
        x0 = self.ball_x
        x, y = x0 + self.vx, self.ball_y + self.vy
        if y < 0:
            y, self.vy = -y, -self.vy
            self.events["wall"] += 1
        elif y > BALL_MAX_Y:
            y, self.vy = 2 * BALL_MAX_Y - y, -self.vy
            self.events["wall"] += 1
        # 4. the paddles
        if self.vx > 0 and x0 + 1 < AGENT_X <= x + 1 and self.agent_y - 1 <= y <= self.agent_y + PADDLE_H - 1:
            off = y + 1 - self.agent_y
            x, self.vx, self.vy = AGENT_X - BALL, -HIT_SPEED[off], HIT_VY[off]
            self.events["hit_agent"] += 1
        elif self.vx < 0 and x0 > OPP_X + 1 >= x and self.opp_y - 1 <= y <= self.opp_y + PADDLE_H - 1:
            off = y + 1 - self.opp_y
            x, self.vx, self.vy = OPP_X + PADDLE_W, HIT_SPEED[off], HIT_VY[off]
            self.events["hit_opp"] += 1
        self.ball_x, self.ball_y = x, y
        # 5. a point
        rew = 0
        if x >= MISS_RIGHT:
            rew = -1
            self.score_opp += 1
            self.events["opp_point"] += 1
        elif x <= MISS_LEFT:
            rew = 1
            self.score_agent += 1
            self.events["agent_point"] += 1
        # 6. the end of the episode, or the serve
        done = (self.score_agent >= self.points_to_win or self.score_opp >= self.points_to_win
                or self.ep_steps >= self.max_episode_steps)
        if done:
            self.over = True
            self.events["episode_end"] += 1
        elif rew != 0:
            self._serve(self._draw(), rew < 0)
        return float(rew), done

    # ---- frames
    def rectangles(self):
        """(x, y, w, h) of the opponent's paddle, the agent's paddle and the ball"""
        return ((OPP_X, self.opp_y, PADDLE_W, PADDLE_H), (AGENT_X, self.agent_y, PADDLE_W, PADDLE_H),
                (self.ball_x, self.ball_y, BALL, BALL))

    def prepped(self):
        """the (1, 80, 80) uint8 frame pong_prep makes of render_rgb(): 1 on the three rectangles, 0 elsewhere"""
        pic = np.zeros((H, W), dtype=np.uint8)
        for x, y, w, h in self.rectangles():
            pic[max(y, 0):y + h, max(x, 0):x + w] = 1
        return pic[None]

    def render_rgb(self):
        pic = np.empty((RAW_H, RAW_W, 3), dtype=np.uint8)
        pic[:] = BORDER_BG
        pic[RAW_TOP:RAW_TOP + 2 * H] = FIELD_BG
        for (x, y, w, h), rgb in zip(self.rectangles(), (OPP_RGB, AGENT_RGB, BALL_RGB)):
            pic[RAW_TOP + 2 * max(y, 0):RAW_TOP + 2 * (y + h), 2 * max(x, 0):2 * (x + w)] = rgb
        return pic


class DevicePongPool(DeviceRegisterWorldPool):
    """``n_envs`` Pong worlds in device memory (the Runner's device-pool protocol).  Env j is the world
    ``PongEnv(seed, env_id=env_id0 + j, ...)``: same draws, same frames; with ``frame_skip`` / ``sticky_num`` / ``sticky_den``
    other than (1, 0, .) a step is an agent step of a2c_pong_step_skip, with ``frame_skip_max`` above
    ``frame_skip`` one of a2c_pong_step_rules (section 6i).  ``device_step`` returns
    ``done = (rew != 0) or real done`` (the Pong override of the reference's runner) and ``reset = real done`` as two tensors.
    ``episode_stats`` counts what the Runner's ``rew_q`` counts for a "Pong" env type: every ``done``, with the reward since
    the last one."""
    WHAT = "Pong"
    frame_shape = (1, H, W)

    def __init__(self, n_envs, device="cuda", seed=0, points_to_win=21, max_episode_steps=10000, opp_skill_num=3,
                 opp_skill_den=4, env_id0=0, frame_skip=1, sticky_num=0, sticky_den=1, frame_skip_max=None):
        world = check_world(points_to_win, max_episode_steps, opp_skill_num, opp_skill_den)
        super().__init__(n_envs, device, seed, env_id0, world, frame_skip, sticky_num, sticky_den, frame_skip_max)


# picklable ``env_fn``: ``PongFactory(env_id=j, **world)()`` is a ``PongEnv``
PongFactory = worlds.factory_of(PongEnv)
FAMILY = worlds.WorldFamily(__name__, "Pong", check_world,
                            (("points_to_win", 21), ("max_episode_steps", 10000), ("opp_skill_num", 3), ("opp_skill_den", 4)),
                            "pong_prep", rule_keys=("frame_skip_max",), pong_done=True, frame_bits=True)
RULE_KEYS, rules_from_hyps, world_from_hyps = FAMILY.rule_keys, FAMILY.rules_from_hyps, FAMILY.world_from_hyps
