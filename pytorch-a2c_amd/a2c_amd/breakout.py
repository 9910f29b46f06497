"""Breakout: the env of BASELINE.json's config 5 (``breakout_prep``, grey frames with more than two levels, real dones
only), as a world that can live in HBM.  The rules are this project's own (parity with ALE is not
claimed), integer arithmetic throughout, implemented twice with the same integers coming out:

  * ``BreakoutEnv``         -- the host twin in NumPy / Python ints with a gym-like surface (``reset()``, ``step(a)``,
                               ``action_space.n == 4``): RAW 210 x 160 x 3 uint8 frames in ALE's layout, which the
                               reference's ``breakout_prep`` turns into the 80 x 72 grey frame ``prepped()`` returns directly;
  * ``DeviceBreakoutPool``  -- ``n_envs`` worlds in device memory stepped by a2c_breakout_step (csrc/breakout.hip): the
                               Runner's device-pool protocol, driven by the actions the sampler wrote.  Frames arrive
                               prepped, grey levels 0..255 as floats.

Field: 72 columns x 80 rows, (x, y) = (column, row), objects named by their top-left pixel.  Bricks: 6 rows x 18 columns,
4 wide x 3 tall, brick (r, c) covers columns 4c..4c+3 and rows 11+3r..13+3r; grey level ROW_LEVEL[r], ROW_POINTS[r]
points.  Paddle: 8 x 2 in rows 77..78, 0 <= px <= 64.  Ball: 2 x 2, 0 <= x <= 70.  Paddle and ball have level 200, the
background 0; a frame shows the bricks, the paddle over them and the ball over both.

One step, in this order (every division below is between non-negative ints):
  1. the agent takes ``a = (action + action_shift) mod 4`` (0 nothing, 1 FIRE = nothing, 2 right, 3 left): the paddle
     moves 3 pixels, clamped to 0..64;
  2. the ball moves by (vx, vy), |vx| and |vy| in {1, 2}; x < 0 -> x = -x, x > 70 -> x = 140 - x, vx = -vx (side walls);
     y < 0 -> y = -y, vy = -vy (ceiling);
  3. brick test on the ball's leading corner at the NEW position, with the velocity as it is after the bounces of 2:
     lx = x + (vx > 0), ly = y + (vy > 0); if 11 <= ly < 29 and brick ((ly - 11) / 3, lx / 4) is alive it dies, the reward
     is its row's points, the ball's y goes back to its OLD y (x keeps the new value), vy = -vy, and for rows 0..2 |vy|
     becomes 2 (it stays 2 until the next serve).  At most one brick per step;
  4. paddle hit: vy > 0, old y + 1 < 77 <= new y + 1 and px - 1 <= x <= px + 7 (the paddle has already moved): the ball
     rests at y = 75, vy = -|vy|, ``off = x + 1 - px`` (0..8) sets vx = HIT_VX[off], where the entry 0 at off = 4 stands
     for +-1 with the sign vx had;
  5. life lost: new y > 78: lives - 1, reward 0;
  6. the episode ends (the REAL done) when lives == 0, or no brick is left, or after ``max_episode_steps`` steps;
     otherwise, after a lost life, the ball is served: one draw ``d``, ball at (8 + d mod 56, 40), vy = -1,
     vx = +1 if (d >> 8) & 1 else -1.
A reset restores all 108 bricks and ``lives`` lives, zeroes the episode-step counter, puts the paddle at px = 32 and
serves with one draw.  Randomness is counter based: draw i of env e is ``hash32(seed, e, i)``, the mixing function of the
Snake and Pong worlds; the only draws are serves.

Frame skip and sticky actions (``frame_skip`` 1..8, ``sticky_num`` / ``sticky_den`` with the bounds of
Pong's ``opp_skill_*``): the step above is one GAME FRAME, and one AGENT step -- ``step(a)`` / ``advance(a)``, one launch
of a2c_breakout_step_skip -- is ``frame_skip`` of them with the same requested action ``a``.  Game frame s = 0 .. k-1:
x = a; when ``sticky_num > 0`` one draw ``d`` is taken BEFORE the frame and x = ``prev`` (the action the previous game
frame executed, state word 17) if ``d mod sticky_den < sticky_num``; prev = x; the frame runs with x and its reward is
added to the agent step's (several bricks may fall in one agent step).  A frame that ends the episode zeroes ``prev``
and the remaining frames are DROPPED (``events["cut"]``).  ``steps``, ``ep_steps`` and ``max_episode_steps`` count game
frames.  With ``sticky_num == 0`` no draw is taken and ``prev`` stays 0: k = 1 is the world above word for word, k > 1 is
that world stepped k times with one action and cut at the done.

Random frame skip, episodic life, reward clipping (a2c_breakout_step_rules):
  * ``frame_skip_max`` (``frame_skip`` .. 8; None = ``frame_skip``): above ``frame_skip`` the agent step first takes ONE draw
    ``d``, before its first sticky draw, and plays k = frame_skip + d mod (frame_skip_max - frame_skip + 1) game frames;
  * ``episodic_life``: a game frame that loses a life WITHOUT ending the episode (rule 5; rule 6 has already served the
    ball) closes the agent step as an episode end does: prev = 0, the remaining frames dropped (``events["cut"]``;
    ``events["life_close"]`` counts the closes), done = 1, ``ep_rew`` zeroed.  The world is not restarted: bricks, lives,
    ``ep_steps`` and its limit carry on, and the ``reset()`` that follows such a done continues the game -- no draw, no
    word changed, the current frame (``continue_episode()`` is its frameless form; ``new_episode()`` stays the full restart);
  * ``clip_rewards``: the agent step's reward is the sign of its sum; ``ep_rew`` keeps the sum itself.

``train()``, env_type "Breakout-device" / "Breakout-host" (the record is ``FAMILY`` below): keys ``lives`` (5),
``max_episode_steps`` (10000), ``frame_skip`` / ``sticky_num`` / ``sticky_den`` / ``frame_skip_max`` as on the Pong worlds, and
for the TRAINING worlds only ``episodic_life`` and ``clip_rewards`` (evaluation plays whole games for the game's score).
``prep_fxn="breakout_prep"`` (grey levels 0..255 on the uint8 transport; with ``hyps["device_prep"] = "breakout_prep"`` on
"Breakout-host" the process pool carries the RAW frames and the device preps them), 4 actions, ``action_shift`` 0 unless
given, real dones only; evaluation on host ``BreakoutEnv``s."""
import numpy as np

from . import worlds
from .worlds import (_M, DeviceRegisterWorldPool, HostWorld, _clamp, _env_id0, _i32, check_repeat, check_rules,  # noqa: F401
                     hash32)

N_ACTIONS = 4
W, H = 72, 80
BRICK_ROWS, BRICK_COLS, BRICK_W, BRICK_H, BRICK_TOP = 6, 18, 4, 3, 11
BRICK_BOTTOM = BRICK_TOP + BRICK_ROWS * BRICK_H                  # 29: the first row below the wall
ROW_LEVEL = (200, 198, 180, 162, 72, 66)                         # channel 0 of ALE's six brick colours, top row first
ROW_POINTS = (7, 7, 4, 4, 1, 1)
ROW_RGB = ((200, 72, 72), (198, 108, 58), (180, 122, 48), (162, 162, 42), (72, 160, 72), (66, 72, 200))
FULL_ROW = (1 << BRICK_COLS) - 1
N_BRICKS = BRICK_ROWS * BRICK_COLS
PADDLE_W, PADDLE_H, PADDLE_Y, PADDLE_SPEED, PADDLE_START_X = 8, 2, 77, 3, 32
PADDLE_MAX_X = W - PADDLE_W
BALL, BALL_MAX_X, LEVEL = 2, W - 2, 200
LOST_Y = 78                                                      # ball y > 78: a life is lost
SERVE_Y, SERVE_X0, SERVE_SPAN = 40, 8, 56
HIT_VX = (-2, -2, -1, -1, 0, 1, 1, 2, 2)                         # by off = ball x + 1 - paddle x; 0: keep the sign, |vx| = 1
MAX_LIVES, MAX_EPISODE_STEPS = 5, 1 << 24
STATE_WORDS = 24
# the kernel's word layout (csrc/breakout.hip): words 11..16 are the brick rows' 18-bit masks, 17 the action of the previous
# game frame (PREV_WORD; 0 without sticky actions), 18..23 spare
PREV_WORD = 17
WORD_NAMES = ("paddle_x", "ball_x", "ball_y", "vx", "vy", "lives_left", "bricks_left", "draws", "steps", "ep_steps", "ep_rew")
# raw frames (ALE's layout): the field is rows 35..194, columns 8..151 at 2 x scale
RAW_H, RAW_W, RAW_TOP, RAW_LEFT, WALL_TOP = 210, 160, 35, 8, 17
WALL_RGB, OBJECT_RGB = (142, 142, 142), (200, 72, 72)


def check_world(lives=5, max_episode_steps=10000, frame_skip=1, sticky_num=0, sticky_den=1, frame_skip_max=None,
                episodic_life=False, clip_rewards=False):
    """the bounds a2c_breakout_step / a2c_breakout_step_skip / a2c_breakout_step_rules enforce (A2C_ERR_ARG): same ones for the
    host twin"""
    n, m = int(lives), int(max_episode_steps)
    check_repeat(frame_skip, sticky_num, sticky_den, "Breakout")
    check_rules(frame_skip, frame_skip_max, episodic_life, clip_rewards, "Breakout", flags=True)
    if not (1 <= n <= MAX_LIVES and 1 <= m <= MAX_EPISODE_STEPS):
        raise ValueError(f"Breakout: unsupported world lives={n} max_episode_steps={m} (1 <= lives <= {MAX_LIVES}, "
                         f"1 <= max_episode_steps <= {MAX_EPISODE_STEPS})")
    return n, m


class _ActionSpace:
    n = N_ACTIONS


class BreakoutEnv(HostWorld):
    """One Breakout world on the host.  ``reset()`` -> raw (210, 160, 3) uint8 frame; ``step(a)`` -> (frame, reward, done,
    info) with the REAL done (no life left, no brick left, or the step limit).  Like a gym env it does not reset itself:
    the caller does -- the Runner does, which yields exactly what the device world returns.  ``events`` counts what
    happened (with frame skip or sticky actions also ``cut``: episode ends that dropped game frames of their agent step, and
    ``sticky``: game frames that kept an action other than the requested one) for tests that must see every rule at work.  ``step`` / ``advance`` are the AGENT
    step: ``frame_skip`` .. ``frame_skip_max`` game frames; with ``episodic_life`` its done is also a lost life, which
    ``reset()`` answers by continuing the game, and with ``clip_rewards`` its reward is a sign (module docstring)."""
    WHAT, N_ACTIONS = "Breakout", N_ACTIONS
    action_space = _ActionSpace()

    def __init__(self, seed=0, env_id=0, lives=5, max_episode_steps=10000, frame_skip=1, sticky_num=0, sticky_den=1,
                 frame_skip_max=None, episodic_life=False, clip_rewards=False):
        self.lives, self.max_episode_steps = check_world(lives, max_episode_steps)
        _, self.episodic_life, self.clip_rewards = check_rules(frame_skip, frame_skip_max, episodic_life, clip_rewards,
                                                               "Breakout", flags=True)
        super().__init__(seed, env_id, frame_skip, sticky_num, sticky_den,
                         ("side_wall", "ceiling", "brick", "speed_up", "paddle_hit", "life_lost", "cleared", "episode_end"),
                         frame_skip_max)
        if self.episodic_life:
            self.events.update(cut=0, sticky=0, life_close=0)
        self._lost = False              # the last game frame lost a life
        self.paddle_x = PADDLE_START_X
        self.ball_x, self.ball_y, self.vx, self.vy = SERVE_X0, SERVE_Y, 1, -1
        self.lives_left, self.bricks_left, self.rows = self.lives, N_BRICKS, [FULL_ROW] * BRICK_ROWS
        self.ep_rew = 0

    def _serve(self):
        d = self._draw()
        self.ball_x, self.ball_y = SERVE_X0 + d % SERVE_SPAN, SERVE_Y
        self.vx, self.vy = (1 if (d >> 8) & 1 else -1), -1

    def new_episode(self):
        """the reset without its frame"""
        self.rows, self.bricks_left, self.lives_left = [FULL_ROW] * BRICK_ROWS, N_BRICKS, self.lives
        self.ep_steps = self.ep_rew = self.prev = 0
        self.paddle_x = PADDLE_START_X
        self._serve()
        self.over = self.closed = False

    def _closes(self):
        """episodic life: the game frame lost a life and the episode goes on"""
        if not (self.episodic_life and self._lost):
            return False
        self.ep_rew = 0
        self.events["life_close"] += 1
        return True

    def advance(self, action):
        total, done = super().advance(action)
        return (float((total > 0) - (total < 0)) if self.clip_rewards else total), done

    def _frame(self, a):
        """one game frame with action ``a`` in 0..3 -> (reward, done)"""
        self.steps += 1
        self.ep_steps += 1
        # 1. the paddle
        self.paddle_x = _clamp(self.paddle_x + (PADDLE_SPEED if a == 2 else (-PADDLE_SPEED if a == 3 else 0)), 0, PADDLE_MAX_X)
        # 2. the ball, the side walls, the ceiling
        y0 = self.ball_y
        x, y = self.ball_x + self.vx, y0 + self.vy
        if x < 0:
            x, self.vx = -x, -self.vx
            self.events["side_wall"] += 1
        elif x > BALL_MAX_X:
            x, self.vx = 2 * BALL_MAX_X - x, -self.vx
            self.events["side_wall"] += 1
        if y < 0:
            y, self.vy = -y, -self.vy
            self.events["ceiling"] += 1
        # 3. the brick under the leading corner
        rew = 0
        lx, ly = x + (self.vx > 0), y + (self.vy > 0)
        if BRICK_TOP <= ly < BRICK_BOTTOM:
            r, c = (ly - BRICK_TOP) // BRICK_H, lx // BRICK_W
            if (self.rows[r] >> c) & 1:
                self.rows[r] &= ~(1 << c)
                self.bricks_left -= 1
                rew = ROW_POINTS[r]
                y, self.vy = y0, -self.vy
                self.events["brick"] += 1
                if r < 3:
                    if abs(self.vy) != 2:
                        self.events["speed_up"] += 1
                    self.vy = 2 if self.vy > 0 else -2
        # 4. the paddle
        if self.vy > 0 and y0 + 1 < PADDLE_Y <= y + 1 and self.paddle_x - 1 <= x <= self.paddle_x + PADDLE_W - 1:
            off = x + 1 - self.paddle_x
            y, self.vy = PADDLE_Y - BALL, -abs(self.vy)
            self.vx = HIT_VX[off] if off != 4 else (1 if self.vx > 0 else -1)
            self.events["paddle_hit"] += 1
        self.ball_x, self.ball_y = x, y
        # 5. a life
        lost = self._lost = y > LOST_Y
        if lost:
            self.lives_left -= 1
            self.events["life_lost"] += 1
        # 6. the end of the episode, or the serve
        self.ep_rew += rew
        done = self.lives_left == 0 or self.bricks_left == 0 or self.ep_steps >= self.max_episode_steps
        if done:
            self.over = True
            self.ep_rew = 0
            self.events["episode_end"] += 1
            if self.bricks_left == 0:
                self.events["cleared"] += 1
        elif lost:
            self._serve()
        return float(rew), done

    # ---- frames
    def prepped(self):
        """the (1, 80, 72) uint8 frame breakout_prep makes of render_rgb(): the bricks' grey levels, 200 on the paddle and
        the ball, 0 elsewhere"""
        pic = np.zeros((H, W), dtype=np.uint8)
        alive = (np.array(self.rows)[:, None] >> np.arange(BRICK_COLS)) & 1                      # (6, 18)
        wall = (alive * np.array(ROW_LEVEL)[:, None]).astype(np.uint8)
        pic[BRICK_TOP:BRICK_BOTTOM] = np.repeat(np.repeat(wall, BRICK_H, axis=0), BRICK_W, axis=1)
        pic[PADDLE_Y:PADDLE_Y + PADDLE_H, self.paddle_x:self.paddle_x + PADDLE_W] = LEVEL
        pic[max(self.ball_y, 0):self.ball_y + BALL, self.ball_x:self.ball_x + BALL] = LEVEL
        return pic[None]

    def render_rgb(self):
        pic = np.zeros((RAW_H, RAW_W, 3), dtype=np.uint8)
        pic[WALL_TOP:RAW_TOP] = WALL_RGB
        pic[WALL_TOP:RAW_TOP + 2 * H, :RAW_LEFT] = WALL_RGB
        pic[WALL_TOP:RAW_TOP + 2 * H, RAW_LEFT + 2 * W:] = WALL_RGB
        field = pic[RAW_TOP:RAW_TOP + 2 * H, RAW_LEFT:RAW_LEFT + 2 * W]
        for r in range(BRICK_ROWS):
            for c in range(BRICK_COLS):
                if (self.rows[r] >> c) & 1:
                    field[2 * (BRICK_TOP + BRICK_H * r):2 * (BRICK_TOP + BRICK_H * (r + 1)),
                          2 * BRICK_W * c:2 * BRICK_W * (c + 1)] = ROW_RGB[r]
        field[2 * PADDLE_Y:2 * (PADDLE_Y + PADDLE_H), 2 * self.paddle_x:2 * (self.paddle_x + PADDLE_W)] = OBJECT_RGB
        field[2 * max(self.ball_y, 0):2 * (self.ball_y + BALL), 2 * self.ball_x:2 * (self.ball_x + BALL)] = OBJECT_RGB
        return pic

    # ---- the kernel's state words
    def state_words(self):
        """this world as the STATE_WORDS int32 words of the device state (WORD_NAMES, the six row masks, spares)"""
        w = np.zeros(STATE_WORDS, dtype=np.int32)
        w[:len(WORD_NAMES)] = [_i32(int(getattr(self, k))) for k in WORD_NAMES]
        w[len(WORD_NAMES):len(WORD_NAMES) + BRICK_ROWS] = self.rows
        w[PREV_WORD] = self.prev
        return w

    def load_state_words(self, words):
        """takes a position from state words (an episode in progress)"""
        w = [int(v) for v in np.asarray(words).reshape(-1)[:STATE_WORDS]]
        for k, v in zip(WORD_NAMES, w):
            setattr(self, k, v & _M if k == "draws" else v)
        self.rows = [v & FULL_ROW for v in w[len(WORD_NAMES):len(WORD_NAMES) + BRICK_ROWS]]
        self.prev = w[PREV_WORD]
        self.over = self.closed = False


class DeviceBreakoutPool(DeviceRegisterWorldPool):
    """``n_envs`` Breakout worlds in device memory (the Runner's device-pool protocol).  Env j is the world
    ``BreakoutEnv(seed, env_id=env_id0 + j, ...)``: same draws, same frames; with ``frame_skip`` / ``sticky_num`` /
    ``sticky_den`` other than (1, 0, .) a step is an agent step of a2c_breakout_step_skip, with
    ``frame_skip_max`` / ``episodic_life`` / ``clip_rewards`` other than (frame_skip, False, False) one of
    a2c_breakout_step_rules (section 6i).  ``device_step`` returns ``done`` and ``reset`` as two tensors holding the same
    values, the real done (with ``episodic_life`` also a lost life).  ``episode_stats`` counts those dones and sums the
    (unclipped) rewards they closed."""
    WHAT, FLAGS = "Breakout", True
    frame_shape = (1, H, W)

    def __init__(self, n_envs, device="cuda", seed=0, lives=5, max_episode_steps=10000, env_id0=0, frame_skip=1, sticky_num=0,
                 sticky_den=1, frame_skip_max=None, episodic_life=False, clip_rewards=False):
        super().__init__(n_envs, device, seed, env_id0, check_world(lives, max_episode_steps), frame_skip, sticky_num, sticky_den,
                         frame_skip_max, episodic_life, clip_rewards)


# picklable ``env_fn``: ``BreakoutFactory(env_id=j, **world)()`` is a ``BreakoutEnv``
BreakoutFactory = worlds.factory_of(BreakoutEnv)
FAMILY = worlds.WorldFamily(__name__, "Breakout", check_world, (("lives", 5), ("max_episode_steps", 10000)), "breakout_prep",
                            rule_keys=worlds.RULE_KEYS, device_prep="breakout_prep")
RULE_KEYS, rules_from_hyps, world_from_hyps, repeat_from_hyps = (FAMILY.rule_keys, FAMILY.rules_from_hyps, FAMILY.world_from_hyps,
                                                                 FAMILY.repeat_from_hyps)
