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
that world stepped k times with one action and cut at the done."""
import numpy as np

from .pong import check_repeat
from .snake import _env_id0, hash32

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
_M = 0xFFFFFFFF


def repeat_from_hyps(hyps):
    """(frame_skip, sticky_num, sticky_den) from the hyps (1, 0, 1 where absent); ValueError outside the bounds"""
    from .pong import repeat_from_hyps as from_hyps
    return from_hyps(hyps, "Breakout")


def check_world(lives=5, max_episode_steps=10000, frame_skip=1, sticky_num=0, sticky_den=1):
    """the bounds a2c_breakout_step / a2c_breakout_step_skip enforce (A2C_ERR_ARG): same ones for the host twin"""
    n, m = int(lives), int(max_episode_steps)
    check_repeat(frame_skip, sticky_num, sticky_den, "Breakout")
    if not (1 <= n <= MAX_LIVES and 1 <= m <= MAX_EPISODE_STEPS):
        raise ValueError(f"Breakout: unsupported world lives={n} max_episode_steps={m} (1 <= lives <= {MAX_LIVES}, "
                         f"1 <= max_episode_steps <= {MAX_EPISODE_STEPS})")
    return n, m


def world_from_hyps(hyps):
    """(lives, max_episode_steps) from the hyps; ValueError outside the bounds"""
    get = lambda k, dflt: dflt if hyps.get(k) is None else hyps[k]
    return check_world(get("lives", 5), get("max_episode_steps", 10000))


def _clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def _i32(v):
    """a 32-bit word as the signed int the device stores"""
    v &= _M
    return v - (1 << 32) if v >> 31 else v


class _ActionSpace:
    n = N_ACTIONS


class BreakoutEnv:
    """One Breakout world on the host.  ``reset()`` -> raw (210, 160, 3) uint8 frame; ``step(a)`` -> (frame, reward, done,
    info) with the REAL done (no life left, no brick left, or the step limit).  Like a gym env it does not reset itself:
    the caller does -- the Runner does, which yields exactly what the device world returns.  ``events`` counts what
    happened (with frame skip or sticky actions also ``cut``: episode ends that dropped game frames of their agent step, and
    ``sticky``: game frames that kept an action other than the requested one) for tests that must see every rule at work.  ``step`` / ``advance`` are the AGENT
    step: ``frame_skip`` game frames (module docstring)."""
    action_space = _ActionSpace()

    def __init__(self, seed=0, env_id=0, lives=5, max_episode_steps=10000, frame_skip=1, sticky_num=0, sticky_den=1):
        self.lives, self.max_episode_steps = check_world(lives, max_episode_steps)
        self.frame_skip, self.sticky_num, self.sticky_den = check_repeat(frame_skip, sticky_num, sticky_den, "Breakout")
        self.prev = 0
        self.seed_, self.env_id = int(seed) & _M, int(env_id)
        self.paddle_x = PADDLE_START_X
        self.ball_x, self.ball_y, self.vx, self.vy = SERVE_X0, SERVE_Y, 1, -1
        self.lives_left, self.bricks_left, self.rows = self.lives, N_BRICKS, [FULL_ROW] * BRICK_ROWS
        self.draws = self.steps = self.ep_steps = self.ep_rew = 0
        self.over = True
        self.events = dict(side_wall=0, ceiling=0, brick=0, speed_up=0, paddle_hit=0, life_lost=0, cleared=0, episode_end=0)
        if (self.frame_skip, self.sticky_num) != (1, 0):      # a plain world can neither cut nor keep an action
            self.events.update(cut=0, sticky=0)

    def seed(self, seed):
        self.seed_ = int(seed) & _M

    def _serve(self):
        d = hash32(self.seed_, self.env_id, self.draws)
        self.draws = (self.draws + 1) & _M
        self.ball_x, self.ball_y = SERVE_X0 + d % SERVE_SPAN, SERVE_Y
        self.vx, self.vy = (1 if (d >> 8) & 1 else -1), -1

    # ---- gym surface
    def reset(self):
        self.new_episode()
        return self.render_rgb()

    def new_episode(self):
        """the reset without its frame"""
        self.rows, self.bricks_left, self.lives_left = [FULL_ROW] * BRICK_ROWS, N_BRICKS, self.lives
        self.ep_steps = self.ep_rew = self.prev = 0
        self.paddle_x = PADDLE_START_X
        self._serve()
        self.over = False

    def step(self, action):
        rew, done = self.advance(action)
        return self.render_rgb(), rew, done, {}

    def advance(self, action):
        """the agent step without its frame: ``frame_skip`` game frames -> (summed reward, done)"""
        if self.over:
            raise RuntimeError("BreakoutEnv.step() after done: call reset()")
        a = int(action) % 4
        total, done = 0.0, False
        for s in range(self.frame_skip):
            x = a
            if self.sticky_num > 0:
                d = hash32(self.seed_, self.env_id, self.draws)
                self.draws = (self.draws + 1) & _M
                if d % self.sticky_den < self.sticky_num:
                    x = self.prev
                    self.events["sticky"] += x != a
                self.prev = x
            rew, done = self._frame(x)
            total += rew
            if done:
                self.prev = 0
                if s < self.frame_skip - 1:
                    self.events["cut"] += 1
                break
        return total, done

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
        lost = y > LOST_Y
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

    def render(self):
        return self.render_rgb()

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
        self.over = False


class BreakoutFactory:
    """picklable ``env_fn`` for ``SequentialEnvironment`` / the env worker processes"""

    def __init__(self, env_id=0, **world):
        self.kw = dict(world, env_id=env_id)

    def __call__(self, *a, **k):
        return BreakoutEnv(**self.kw)


class DeviceBreakoutPool:
    """``n_envs`` Breakout worlds in device memory (the Runner's device-pool protocol).  Env j is the world
    ``BreakoutEnv(seed, env_id=env_id0 + j, ...)``: same draws, same frames; with ``frame_skip`` / ``sticky_num`` /
    ``sticky_den`` other than (1, 0, .) a step is an agent step of a2c_breakout_step_skip.  ``device_step`` returns ``done`` and ``reset`` as two
    tensors holding the same values, the real done.  ``episode_stats`` counts the finished episodes and sums their rewards."""
    needs_actions = True
    frame_shape = (1, H, W)

    def __init__(self, n_envs, device="cuda", seed=0, lives=5, max_episode_steps=10000, env_id0=0, frame_skip=1, sticky_num=0,
                 sticky_den=1):
        import torch
        from . import ops
        self.world = check_world(lives, max_episode_steps)
        self.repeat = check_repeat(frame_skip, sticky_num, sticky_den, "Breakout")
        self.plain = self.repeat[:2] == (1, 0)      # today's world: the entry points without frame skip
        self.B, self.seed, self.device = int(n_envs), int(seed) & _M, torch.device(device)
        if self.B < 1:
            raise ValueError("DeviceBreakoutPool: n_envs >= 1")
        self.env_id0 = _env_id0(env_id0, self.B)
        self.HW = H * W
        self.words = ops.breakout_state_bytes(self.world[0]) // 4
        dev = self.device
        self.state = torch.zeros((self.B, self.words), dtype=torch.int32, device=dev)
        self.frames = torch.zeros((self.B, self.HW), dtype=torch.float32, device=dev)
        self.rew, self.done, self.reset_mask = (torch.zeros(self.B, dtype=torch.float32, device=dev) for _ in range(3))
        self.ep_stats = torch.zeros(2, dtype=torch.int32, device=dev)      # episodes finished, sum of their rewards
        self.action_shift = 0
        self.started = False

    def __len__(self):
        return self.B

    def reset_all(self, env_id0=None):
        """(re)starts every world: counters to 0, then the serve draw; state and frames of the reset positions.  ``env_id0``
        re-bases the pool first: env j becomes world ``env_id0 + j``"""
        from . import ops
        if env_id0 is not None:
            self.env_id0 = _env_id0(env_id0, self.B)
        ops.breakout_reset(self.state, self.B, self.env_id0, self.seed, *self.world, self.frames, self.HW)
        self.started = True

    def start(self, runner):
        import torch
        from . import ops
        self.action_shift = int(runner.hyps["action_shift"])
        self.reset_all()
        ones = torch.ones(self.B, dtype=torch.float32, device=self.device)
        ops.frame_stack_push(self.frames, ones, runner.bookmark.data_ptr(), runner.S, runner.bookmark.data_ptr(), runner.S,
                             self.B, runner.C, runner.HW)

    def step(self, actions_ptr, act_stride, env0=0, B=None):
        """advance envs env0..env0+B by the int64 actions at ``actions_ptr`` (element stride ``act_stride``)"""
        from . import ops
        B = self.B - env0 if B is None else B
        if not self.started:
            raise RuntimeError("DeviceBreakoutPool: reset_all() / start(runner) first")
        if env0 < 0 or B < 1 or env0 + B > self.B:
            raise ValueError("DeviceBreakoutPool: env range outside the pool")
        sl = slice(env0, env0 + B)
        if self.plain:
            ops.breakout_step(self.state[sl], actions_ptr, act_stride, self.action_shift, B, self.env_id0 + env0,
                              self.seed, *self.world, self.frames[sl], self.HW, self.rew[sl], self.done[sl],
                              self.reset_mask[sl], self.ep_stats[0:1], self.ep_stats[1:2])
        else:
            ops.breakout_step_skip(self.state[sl], actions_ptr, act_stride, self.action_shift, B, self.env_id0 + env0,
                                   self.seed, *self.world, self.frames[sl], self.HW, self.rew[sl], self.done[sl],
                                   self.reset_mask[sl], *self.repeat, self.ep_stats[0:1], self.ep_stats[1:2])
        return self.frames[sl], self.rew[sl], self.done[sl], self.reset_mask[sl]

    def device_step(self, t, env0, B, actions=None):
        if actions is None:
            raise ValueError("DeviceBreakoutPool.device_step needs actions=(address, stride)")
        return self.step(actions[0], actions[1], env0, B)

    def device_step_post(self, t, env0, B, actions, post, frames=False):
        """``device_step`` + the bookkeeping of env step ``t`` + the frame stack in ONE launch (a2c_breakout_step_post): ``post`` is
        an ``ops.world_post`` block.  The new frame goes into plane C - 1 of ``post.out``; ``self.frames`` is written as
        well only with ``frames=True`` (the Runner does not read it).  -> (rew, done, reset)"""
        from . import ops
        if not self.started:
            raise RuntimeError("DeviceBreakoutPool: reset_all() / start(runner) first")
        if env0 < 0 or B < 1 or env0 + B > self.B:
            raise ValueError("DeviceBreakoutPool: env range outside the pool")
        sl = slice(env0, env0 + B)
        if self.plain:
            ops.breakout_step_post(self.state[sl], actions[0], actions[1], self.action_shift, B, self.env_id0 + env0,
                                   self.seed, *self.world, self.frames[sl] if frames else None, self.HW, self.rew[sl],
                                   self.done[sl], self.reset_mask[sl], post, self.ep_stats[0:1], self.ep_stats[1:2])
        else:
            ops.breakout_step_post_skip(self.state[sl], actions[0], actions[1], self.action_shift, B, self.env_id0 + env0,
                                        self.seed, *self.world, self.frames[sl] if frames else None, self.HW, self.rew[sl],
                                        self.done[sl], self.reset_mask[sl], *self.repeat, post, self.ep_stats[0:1],
                                        self.ep_stats[1:2])
        return self.rew[sl], self.done[sl], self.reset_mask[sl]

    def episode_stats(self):
        """(episodes finished, sum of their rewards) since the last call; one device read"""
        n, s = (int(v) for v in self.ep_stats.tolist())
        if n:
            self.ep_stats.zero_()
        return n, s
