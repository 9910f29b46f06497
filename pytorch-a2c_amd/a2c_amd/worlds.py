"""What the worlds that can live in HBM (snake.py, pong.py, breakout.py) share on the Python side: the counter-based draws,
the bounds of frame skip and sticky actions, ``HostWorld`` -- the agent step of the host twins ``PongEnv`` / ``BreakoutEnv`` --
and ``DeviceWorldPool``, the Runner's device-pool protocol over ``n_envs`` worlds in device memory (the kernels' side:
csrc/world.h), with ``DeviceLaneWorldPool``, what the pools of the one-lane-per-env worlds (point.py,
cartpole.py, pendulum.py; csrc/lane_world.h) share beyond it."""
import functools
import math

_M = 0xFFFFFFFF
MAX_FRAME_SKIP, MAX_STICKY_DEN = 8, 1 << 16


def _fin(x):
    """the integer finaliser (lowbias32): x ^= x>>16; x *= 0x7FEB352D; x ^= x>>15; x *= 0x846CA68B; x ^= x>>16 (mod 2^32)"""
    x &= _M
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M
    x ^= x >> 16
    return x


def hash32(seed, env_id, draw_index):
    """fin(fin(fin(seed + 0x9E3779B9) ^ env_id) ^ draw_index), everything mod 2^32"""
    return _fin(_fin(_fin((int(seed) + 0x9E3779B9) & _M) ^ (int(env_id) & _M)) ^ (int(draw_index) & _M))


def _env_id0(env_id0, B):
    """first env id of a pool of B worlds: the kernels take ids as non-negative C ints"""
    v = int(env_id0)
    if v < 0 or v + int(B) > 0x7FFFFFFF:
        raise ValueError(f"env_id0={env_id0}: env ids are 0 .. 2^31 - 1")
    return v


def _clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def _i32(v):
    """a 32-bit word as the signed int the device stores"""
    v &= _M
    return v - (1 << 32) if v >> 31 else v


def check_repeat(frame_skip=1, sticky_num=0, sticky_den=1, what="Pong", frame_skip_max=None):
    """the bounds a2c_<world>_step_skip / _step_rules enforce (A2C_ERR_ARG) on frame skip (``frame_skip_max``: None, or
    frame_skip .. 8) and sticky actions: same ones for the host twins -> (frame_skip, sticky_num, sticky_den)"""
    k, n, d = int(frame_skip), int(sticky_num), int(sticky_den)
    if not (1 <= k <= MAX_FRAME_SKIP and 1 <= d <= MAX_STICKY_DEN and 0 <= n <= d):
        raise ValueError(f"{what}: unsupported frame_skip={k} sticky={n}/{d} (1 <= frame_skip <= {MAX_FRAME_SKIP}, "
                         f"1 <= sticky_den <= {MAX_STICKY_DEN}, 0 <= sticky_num <= sticky_den)")
    if frame_skip_max is not None and not k <= int(frame_skip_max) <= MAX_FRAME_SKIP:
        raise ValueError(f"{what}: unsupported frame_skip_max={frame_skip_max} (frame_skip = {k} <= frame_skip_max <= "
                         f"{MAX_FRAME_SKIP})")
    return k, n, d


def check_rules(frame_skip=1, frame_skip_max=None, episodic_life=False, clip_rewards=False, what="Pong", flags=False):
    """the bounds a2c_<world>_step_rules enforces on what DESIGN.md section 6i adds; ``flags``: the world has episodic_life /
    clip_rewards (Breakout) -> (frame_skip_max, episodic_life, clip_rewards), ``frame_skip_max`` None becoming ``frame_skip``"""
    k = check_repeat(frame_skip, what=what, frame_skip_max=frame_skip_max)[0]
    out = []
    for name, v in (("episodic_life", episodic_life), ("clip_rewards", clip_rewards)):
        v = 0 if v is None else v
        if isinstance(v, str) or v not in (0, 1):
            raise ValueError(f"{what}: {name}={v!r} is neither 0 nor 1")
        if v and not flags:
            raise ValueError(f"{what}: {name} is a key of the Breakout worlds ({what} closes its steps and bounds its rewards "
                             "by its own rules)")
        out.append(bool(v))
    return (k if frame_skip_max is None else int(frame_skip_max), *out)


RULE_KEYS = ("frame_skip_max", "episodic_life", "clip_rewards")


def repeat_from_hyps(hyps, what="Pong"):
    """(frame_skip, sticky_num, sticky_den) from the hyps (1, 0, 1 where absent); ValueError outside the bounds, those of a
    ``frame_skip_max`` among the hyps included"""
    get = lambda k, dflt: dflt if hyps.get(k) is None else hyps[k]
    return check_repeat(get("frame_skip", 1), get("sticky_num", 0), get("sticky_den", 1), what, hyps.get("frame_skip_max"))


def rules_from_hyps(hyps, what="Pong", keys=RULE_KEYS):
    """{key: value} of the keys of RULE_KEYS this world family takes (``keys``), defaults where absent; ValueError outside the
    bounds and for a key of RULE_KEYS the family does not take"""
    get = lambda k, dflt: dflt if hyps.get(k) is None else hyps[k]
    alien = [k for k in RULE_KEYS if k not in keys and hyps.get(k) is not None and (k == "frame_skip_max" or hyps[k] != 0)]
    if alien:
        raise ValueError(f"a2c_amd: {', '.join(alien)}: not a key of the {what} worlds (frame_skip_max: Pong and Breakout; "
                         "episodic_life, clip_rewards: Breakout)")
    vals = check_rules(get("frame_skip", 1), hyps.get("frame_skip_max"), get("episodic_life", False),
                       get("clip_rewards", False), what, flags="episodic_life" in keys)
    return {k: v for k, v in zip(RULE_KEYS, vals) if k in keys}


class HostWorld:
    """The gym-like surface and the AGENT step of the host twins of the register worlds (csrc/world.h):
    ``frame_skip`` .. ``frame_skip_max`` game frames with sticky actions (the module docstrings of pong.py / breakout.py state
    the rules).  A subclass supplies ``WHAT`` (its name in messages), ``N_ACTIONS``, ``new_episode()``, ``_frame(a)`` ->
    (reward, done), ``render_rgb()`` and, where an agent step has an invariant, ``_check_step(total)``; where something other
    than an episode end closes an agent step, ``_closes()``."""
    WHAT, N_ACTIONS = "World", 1

    def __init__(self, seed, env_id, frame_skip, sticky_num, sticky_den, events, frame_skip_max=None):
        self.frame_skip, self.sticky_num, self.sticky_den = check_repeat(frame_skip, sticky_num, sticky_den, self.WHAT,
                                                                         frame_skip_max)
        self.frame_skip_max = self.frame_skip if frame_skip_max is None else int(frame_skip_max)
        self.prev = 0
        self.last_k = 0                 # game frames the last agent step was to play (rule 1)
        self.seed_, self.env_id = int(seed) & _M, int(env_id)
        self.draws = self.steps = self.ep_steps = 0
        self.over = True
        self.closed = False             # the last agent step closed without ending the episode: reset() continues the game
        self.events = dict.fromkeys(events, 0)
        if (self.frame_skip_max, self.sticky_num) != (1, 0):      # a plain world can neither cut nor keep an action
            self.events.update(cut=0, sticky=0)

    def seed(self, seed):
        self.seed_ = int(seed) & _M

    def _draw(self):
        d = hash32(self.seed_, self.env_id, self.draws)
        self.draws = (self.draws + 1) & _M
        return d

    # ---- gym surface
    def reset(self):
        """after a done that closed an agent step without ending the episode (``closed``): the game goes on -- no draw, no
        state changed, the current frame (what baselines' EpisodicLifeEnv does); else the full restart"""
        if self.closed:
            self.continue_episode()
        else:
            self.new_episode()
        return self.render_rgb()

    def continue_episode(self):
        """the continuing reset without its frame: takes up the game where a close that was no episode end left it"""
        if self.over or not self.closed:
            raise RuntimeError(f"{self.WHAT}Env.continue_episode(): the last step did not close inside an episode")
        self.closed = False

    def step(self, action):
        rew, done = self.advance(action)
        return self.render_rgb(), rew, done, {}

    def render(self):
        return self.render_rgb()

    def advance(self, action):
        """the agent step without its frame: k game frames -> (summed reward, done), k = ``frame_skip``, or with
        ``frame_skip_max`` above it ONE draw d taken first: k = frame_skip + d mod (frame_skip_max - frame_skip + 1)"""
        if self.over or self.closed:
            raise RuntimeError(f"{self.WHAT}Env.step() after done: call reset()")
        a = self._action(action)
        k = self.frame_skip
        if self.frame_skip_max > k:
            k += self._draw() % (self.frame_skip_max - k + 1)
        self.last_k = k
        total, done = 0.0, False
        for s in range(k):
            x = a
            if self.sticky_num > 0:
                if self._draw() % self.sticky_den < self.sticky_num:
                    x = self.prev
                    self.events["sticky"] += x != a
                self.prev = x
            rew, done = self._frame(x)
            total += rew
            self.closed = not done and self._closes()
            if done or self.closed:
                self.prev = 0
                if s < k - 1:
                    self.events["cut"] += 1
                break
        self._check_step(total)
        return total, done or self.closed

    def _action(self, action):
        """what ``step`` was handed as the int the game frames take: ``action mod N_ACTIONS``; a world with float actions
        (point.py) packs its quantised components instead.  0 must be the action ``prev`` holds after an episode end"""
        return int(action) % self.N_ACTIONS

    def _check_step(self, total):
        pass

    def _closes(self):
        """after a game frame that did not end the episode: does it close the agent step all the same?"""
        return False


class LaneHostWorld(HostWorld):
    """``HostWorld`` of the twins of the lane worlds (point.py, cartpole.py, pendulum.py): every ``step()`` also sets
    ``truncated`` -- the step ended the episode at a game frame where the step limit held and the game's own end condition did
    not (``_frame`` says so in ``limit_alone``; both at one frame is a terminal end) -- and ``final_obs``, the observation of
    the world the episode ended in.  A twin does not restart itself, so that is the step's own observation, ended or not: what
    a2c_<world>_step_trunc reports beside a step whose world HAS restarted.  ``step()``'s return value
    and ``info`` are what they were."""
    truncated, final_obs, limit_alone = False, None, False

    def step(self, action):
        self.limit_alone = False
        out = super().step(action)
        self.truncated = bool(out[2] and self.limit_alone)
        self.final_obs = out[0].copy()
        return out


class WorldFactory:
    """picklable ``env_fn`` for ``SequentialEnvironment`` / the env worker processes: ``env(env_id=..., **world)``"""

    def __init__(self, env, env_id=0, **world):
        self.env, self.kw = env, dict(world, env_id=env_id)

    def __call__(self, *a, **k):
        return self.env(**self.kw)


def factory_of(env):
    """``WorldFactory`` with its env class bound: ``factory_of(PongEnv)(env_id=3, seed=1)()`` is a ``PongEnv``"""
    return functools.partial(WorldFactory, env)


class DeviceWorldPool:
    """``n_envs`` worlds in device memory (the Runner's device-pool protocol: ``start`` / ``device_step`` /
    ``device_step_post``).  ``needs_actions``: the Runner hands ``device_step`` the address and stride of the int64 actions the
    sampler just wrote.  A subclass checks its world in ``__init__``, sets ``frame_shape`` and makes the library calls in
    ``_reset()`` and ``_step(head, out, frames, post, sl)``."""
    needs_actions = True
    MIN_ENVS = 1

    def __init__(self, n_envs, device, seed, env_id0, words):
        import torch
        self.B, self.seed, self.device = int(n_envs), int(seed) & _M, torch.device(device)
        if self.B < self.MIN_ENVS:
            raise ValueError(f"{type(self).__name__}: n_envs >= {self.MIN_ENVS}")
        self.env_id0 = _env_id0(env_id0, self.B)
        self.HW = math.prod(self.frame_shape[1:])          # (1, H, W) pictures, or a (1, L) vector
        self.words = words
        dev = self.device
        self.state = torch.zeros((self.B, self.words), dtype=torch.int32, device=dev)
        self.frames = torch.zeros((self.B, self.HW), dtype=torch.float32, device=dev)
        self.rew, self.done, self.reset_mask = (torch.zeros(self.B, dtype=torch.float32, device=dev) for _ in range(3))
        self.ep_stats = torch.zeros(2, dtype=torch.int32, device=dev)      # dones, sum of the rewards they closed
        self.action_shift = 0
        self.started = False

    def __len__(self):
        return self.B

    def reset_all(self, env_id0=None):
        """(re)starts every world: counters to 0, then the reset draws; state and frames of the reset positions.  ``env_id0``
        re-bases the pool first: env j becomes world ``env_id0 + j``"""
        if env_id0 is not None:
            self.env_id0 = _env_id0(env_id0, self.B)
        self._reset()
        self.started = True

    def start(self, runner):
        import torch
        from . import ops
        self.action_shift = int(runner.hyps["action_shift"])
        self.reset_all()
        ones = torch.ones(self.B, dtype=torch.float32, device=self.device)
        ops.frame_stack_push(self.frames, ones, runner.bookmark.data_ptr(), runner.S, runner.bookmark.data_ptr(), runner.S,
                             self.B, runner.C, runner.HW)

    def _launch(self, actions_ptr, act_stride, env0, B, frames, post, trunc=None):
        """one launch over envs env0..env0+B: the arguments every world's step begins with, and its three outputs.  ``trunc``:
        an ``ops.world_trunc`` block (the lane worlds, hyps bootstrap_truncated: DESIGN.md section 6o) or None"""
        if not self.started:
            raise RuntimeError(f"{type(self).__name__}: reset_all() / start(runner) first")
        if env0 < 0 or B < 1 or env0 + B > self.B:
            raise ValueError(f"{type(self).__name__}: env range outside the pool")
        sl = slice(env0, env0 + B)
        head = (self.state[sl], actions_ptr, act_stride, self.action_shift, B, self.env_id0 + env0, self.seed)
        out = (self.rew[sl], self.done[sl], self.reset_mask[sl])
        if trunc is None:
            self._step(head, out, self.frames[sl] if frames else None, post, sl)
        elif not self.reports_trunc:
            raise ValueError(f"bootstrap_truncated: {type(self).__name__} does not report the state an episode ended in (the "
                             "lane worlds do: Point, CartPole, Pendulum)")
        else:
            self._step(head, out, self.frames[sl] if frames else None, post, sl, trunc=trunc)
        return out

    reports_trunc = False          # has a2c_<world>_step_trunc (DeviceLaneWorldPool)

    def step(self, actions_ptr, act_stride, env0=0, B=None, trunc=None):
        """advance envs env0..env0+B by the int64 actions at ``actions_ptr`` (element stride ``act_stride``)"""
        B = self.B - env0 if B is None else B
        return (self.frames[env0:env0 + B],) + self._launch(actions_ptr, act_stride, env0, B, True, None, trunc)

    def device_step(self, t, env0, B, actions=None, trunc=None):
        if actions is None:
            raise ValueError(f"{type(self).__name__}.device_step needs actions=(address, stride)")
        return self.step(actions[0], actions[1], env0, B, trunc)

    def device_step_post(self, t, env0, B, actions, post, frames=False, trunc=None):
        """``device_step`` + the bookkeeping of env step ``t`` + the frame stack in ONE launch (a2c_<world>_step_post): ``post``
        is an ``ops.world_post`` block.  The new frame goes into plane C - 1 of ``post.out``; ``self.frames`` is written as
        well only with ``frames=True`` (the Runner does not read it).  -> (rew, done, reset)"""
        return self._launch(actions[0], actions[1], env0, B, frames, post, trunc)

    def episode_stats(self):
        """(dones, sum of the rewards they closed) since the last call; one device read"""
        n, s = (int(v) for v in self.ep_stats.tolist())
        if n:
            self.ep_stats.zero_()
        return n, s


class DeviceLaneWorldPool(DeviceWorldPool):
    """The pools of the worlds where ONE LANE plays an env (csrc/lane_world.h: point.py, cartpole.py, pendulum.py), whose library
    calls differ in their name and in the world's parameters alone.  A subclass sets ``WHAT`` (its name in messages; lower-cased,
    the prefix of ``ops.<what>_state_bytes / _reset / _step``), ``frame_shape`` and, where the actions are float rows,
    ``float_actions`` and ``n_act``; its ``__init__`` hands over its checked ``world`` tuple, the parameters in the order the
    library takes them."""
    WHAT = "World"
    reports_trunc = True

    def __init__(self, n_envs, device, seed, env_id0, world, frame_skip, sticky_num, sticky_den, frame_skip_max):
        from . import ops
        self.world = world
        self.repeat = check_repeat(frame_skip, sticky_num, sticky_den, self.WHAT)
        self.rules = ops.world_rules(*self.repeat, *check_rules(frame_skip, frame_skip_max, what=self.WHAT), always=True)
        self._op = {f: getattr(ops, f"{self.WHAT.lower()}_{f}") for f in ("state_bytes", "reset", "step", "step_trunc")}
        super().__init__(n_envs, device, seed, env_id0, self._op["state_bytes"]() // 4)
        self._shift = float if getattr(self, "float_actions", False) else int
        self.action_shift = self._shift(0)

    def start(self, runner):
        super().start(runner)
        self.action_shift = self._shift(runner.hyps["action_shift"])      # (the base class keeps the int of the discrete worlds)

    def _reset(self):
        self._op["reset"](self.state, self.B, self.env_id0, self.seed, *self.world, self.frames, self.HW)

    def _step(self, head, out, frames, post, sl, trunc=None):
        tail = (self.rules, post, self.ep_stats[0:1], self.ep_stats[1:2])
        if trunc is None:
            self._op["step"](*head, *self.world, frames, self.HW, *out, *tail)
        else:
            self._op["step_trunc"](*head, *self.world, frames, self.HW, *out, trunc, *tail)
