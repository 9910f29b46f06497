"""Snake: the third env family of the reference (gym-snake, ``snake_prep``), as a world that can live in HBM.

Two implementations of ONE set of rules (DESIGN.md "Snake"), which produce the same integers:

  * ``SnakeEnv``         -- the host twin in NumPy with a gym-like surface (``reset()``, ``step(a)``,
                            ``action_space.n == 4``, raw RGB frames), usable behind ``SequentialEnvironment(env_fn=...)``,
                            ``HostEnvPool``, ``ProcessEnvPool`` and ``StatsRunner``;
  * ``DeviceSnakePool``  -- ``n_envs`` worlds in device memory stepped by a2c_snake_step (csrc/snake.hip): the Runner's
                            device-pool protocol (``start`` / ``device_step``), driven by the actions the sampler wrote.
                            Frames arrive already prepped (``snake_prep``'s values); a whole rollout is enqueued without
                            a host synchronisation and can be captured: the draw counters live in device memory.

Rules.  G x G cells, every cell a u x u block of one colour: space [0,255,0], body [1,0,0], head [255,0,0], food
[0,0,255].  Actions 0 up, 1 right, 2 down, 3 left (``(action + action_shift) & 3``); the head moves one cell per step.
Leaving the grid or entering a body cell (neck and tail cell included: the tail is vacated after the move) ends the
episode with reward -1.  Entering a food cell gives +1, the snake grows by one and a new food appears on a free cell; if
no free cell is left the grid is full and the episode ends (with that step's +1).  Every other move gives 0.  A reset
draws heading and head cell, lays a snake of length 3 behind the head and places ``n_foods`` foods.  After a done the env
resets itself: the frame returned is the reset frame and ``reset == done``.

Randomness is counter based: draw number i of env e is ``hash32(seed, e, i)`` (below); a free cell is the k-th free cell
in row-major order with ``k = draw mod n_free``.  The body is a time-to-live map: a cell holds 0 (free), -1 (food) or the
number of steps it stays occupied (head = length).

``train()``, env_type "Snake-device" / "Snake-host" (the record is ``FAMILY`` below): the reference's keys ``grid_size`` (15;
an int or [g, g]), ``unit_size`` (4), ``n_foods`` (2); ``prep_fxn="snake_prep"``, 4 actions; one game frame per step, so
``frame_skip`` / ``sticky_num`` and the three keys of DESIGN.md section 6i are a ValueError; evaluation on host ``SnakeEnv``s."""
import numpy as np

from .worlds import _M, DeviceWorldPool, WorldFamily, _env_id0, _fin, factory_of, hash32  # noqa: F401

N_ACTIONS = 4
DR = (-1, 0, 1, 0)
DC = (0, 1, 0, -1)
SPACE, BODY, HEAD, FOOD = (0, 255, 0), (1, 0, 0), (255, 0, 0), (0, 0, 255)
PREP_SPACE, PREP_BODY, PREP_HEAD, PREP_FOOD = 0.0, 1.0, 1.5, .33          # what snake_prep makes of the four colours


def check_world(grid_size, unit_size, n_foods):
    """the bounds a2c_snake_step enforces (A2C_ERR_ARG): same ones for the host twin"""
    G, u, nf = int(grid_size), int(unit_size), int(n_foods)
    if not (4 <= G <= 32 and 1 <= u <= 16 and ((G * u) ** 2) % 4 == 0 and 1 <= nf < G * G - 3):
        raise ValueError(f"Snake: unsupported world grid_size={G} unit_size={u} n_foods={nf} (4 <= grid_size <= 32, "
                         "1 <= unit_size <= 16, (grid_size*unit_size)^2 a multiple of 4, 1 <= n_foods < grid_size^2 - 3)")
    return G, u, nf


def _world_from_hyps(hyps):
    """(grid_size, unit_size, n_foods) from the reference's keys (``grid_size`` may be an int or [g, g])"""
    g = hyps.get("grid_size", 15)
    if isinstance(g, (list, tuple)):
        if len(g) != 2 or g[0] != g[1]:
            raise ValueError("Snake: grid_size must be square")
        g = g[0]
    return check_world(15 if g is None else g, hyps.get("unit_size", 4) or 4, hyps.get("n_foods", 2) or 2)


class _ActionSpace:
    n = N_ACTIONS


class SnakeEnv:
    """One Snake world on the host.  ``reset()`` -> raw (G*u, G*u, 3) uint8 frame; ``step(a)`` -> (frame, reward, done,
    info).  Like a gym env it does NOT reset itself: ``frame`` after a done is the terminal position's (a dead snake
    stays where it was) and the caller resets -- the Runner does, which yields exactly what the device world returns."""
    action_space = _ActionSpace()

    def __init__(self, seed=0, env_id=0, grid_size=15, unit_size=4, n_foods=2):
        self.G, self.u, self.n_foods = check_world(grid_size, unit_size, n_foods)
        self.seed_, self.env_id = int(seed) & _M, int(env_id)
        self.cells = np.zeros((self.G, self.G), dtype=np.int32)
        self.head, self.length, self.draws, self.steps = (0, 0), 0, 0, 0
        self.over = True

    def seed(self, seed):
        self.seed_ = int(seed) & _M

    # ---- randomness
    def _draw(self):
        d = hash32(self.seed_, self.env_id, self.draws)
        self.draws = (self.draws + 1) & _M
        return d

    def _place_food(self, n_free):
        """food on the k-th free cell in row-major order, k = draw mod n_free"""
        k = self._draw() % n_free
        free = np.flatnonzero(self.cells.reshape(-1) == 0)
        assert len(free) == n_free, (len(free), n_free)
        self.cells.reshape(-1)[free[k]] = -1

    # ---- gym surface
    def reset(self):
        G = self.G
        self.cells[:] = 0
        h = self._draw() & 3
        k = self._draw() % ((G - 2) * G)
        a, b = k // G, k % G                   # a: along the heading's axis (room for the body behind), b: across
        if h == 0:
            r, c = a, b
        elif h == 1:
            r, c = b, a + 2
        elif h == 2:
            r, c = a + 2, b
        else:
            r, c = b, a
        for i in range(3):                     # head = 3, then 2, 1 behind it
            self.cells[r - i * DR[h], c - i * DC[h]] = 3 - i
        self.head, self.length, self.over = (r, c), 3, False
        for i in range(self.n_foods):
            self._place_food(G * G - 3 - i)
        return self.render_rgb()

    def step(self, action):
        if self.over:
            raise RuntimeError("SnakeEnv.step() after done: call reset()")
        a = int(action) & 3
        G, cells = self.G, self.cells
        r, c = self.head[0] + DR[a], self.head[1] + DC[a]
        self.steps += 1
        if not (0 <= r < G and 0 <= c < G) or cells[r, c] > 0:
            self.over = True
            return self.render_rgb(), -1.0, True, {}
        if cells[r, c] < 0:                    # food: grow, no cell is vacated
            self.length += 1
            cells[r, c] = self.length
            self.head = (r, c)
            n_free = G * G - self.length - (self.n_foods - 1)
            if n_free == 0:                    # the grid is full
                self.over = True
                return self.render_rgb(), 1.0, True, {}
            self._place_food(n_free)
            return self.render_rgb(), 1.0, False, {}
        cells[cells > 0] -= 1                  # the tail cell is vacated AFTER the move was judged
        cells[r, c] = self.length
        self.head = (r, c)
        return self.render_rgb(), 0.0, False, {}

    def render(self):
        return self.render_rgb()

    # ---- frames
    def render_rgb(self):
        c = self.cells
        pic = np.empty((self.G, self.G, 3), dtype=np.uint8)
        pic[:] = SPACE
        pic[c > 0] = BODY
        pic[c < 0] = FOOD
        pic[(c == self.length) & (c > 0)] = HEAD
        return np.ascontiguousarray(pic.repeat(self.u, axis=0).repeat(self.u, axis=1))


class DeviceSnakePool(DeviceWorldPool):
    """``n_envs`` Snake worlds in device memory (the Runner's device-pool protocol).  Env j is the world
    ``SnakeEnv(seed, env_id=env_id0 + j, ...)``: same draws, same frames (with ``raw_frames`` also the raw RGB ones, ``rgb``)."""

    MIN_ENVS = 0      # a pool of no worlds constructs and resets (a2c_snake_reset accepts B == 0), as it always did

    def __init__(self, n_envs, device="cuda", seed=0, grid_size=15, unit_size=4, n_foods=2, raw_frames=False, env_id0=0):
        import torch
        from . import ops
        self.G, self.u, self.n_foods = check_world(grid_size, unit_size, n_foods)
        side = self.G * self.u
        self.frame_shape = (1, side, side)
        super().__init__(n_envs, device, seed, env_id0, ops.snake_state_bytes(self.G, self.n_foods) // 4)
        self.rgb = torch.zeros((self.B, side, side, 3), dtype=torch.uint8, device=self.device) if raw_frames else None

    reset = DeviceWorldPool.reset_all

    def _reset(self):
        from . import ops
        ops.snake_reset(self.state, self.B, self.env_id0, self.seed, self.G, self.u, self.n_foods, self.frames, self.rgb)

    def _step(self, head, out, frames, post, sl):
        from . import ops
        rgb = None if self.rgb is None else self.rgb[sl]
        if post is None:
            ops.snake_step(*head, self.G, self.u, self.n_foods, *out, frames, rgb, self.ep_stats)
        else:
            ops.snake_step_post(*head, self.G, self.u, self.n_foods, *out, frames, post, rgb, self.ep_stats)


def _frame_shape(world):
    side = world["grid_size"] * world["unit_size"]
    return 1, side, side


# picklable ``env_fn`` for ``SequentialEnvironment`` / the env worker processes: ``SnakeFactory(env_id=j, **world)()``
SnakeFactory = factory_of(SnakeEnv)
# the family record (worlds.WorldFamily): one game frame per step, none of the rule keys of DESIGN.md section 6i
FAMILY = WorldFamily(__name__, "Snake", check_world, (("grid_size", 15), ("unit_size", 4), ("n_foods", 2)), "snake_prep",
                     repeats=False, world_from_hyps=_world_from_hyps, frame_shape=_frame_shape)
world_from_hyps = FAMILY.world_from_hyps
