"""Point on the host (no GPU needed): ``a2c_amd.point.PointEnv`` against an agent-step loop written
out here, value for value; the action quantiser on its edge values; an action stream that shows every rule at work; the
bounds of the world, pool, twin and ``train()`` keys.  The device worlds are compared with this host twin in
test_gpu_point.py, which plays the streams built here."""
import functools
import pickle

import numpy as np
import pytest

from a2c_amd import point
from a2c_amd.point import PointEnv, PointFactory, quantise, world_from_hyps
from a2c_amd.worlds import hash32

PLAIN = dict()
REPEAT = dict(frame_skip=2, frame_skip_max=4, sticky_num=1, sticky_den=4)          # (2, 4, sticky 1/4)
RULES = {"plain": PLAIN, "repeat": REPEAT}
WORLD = dict(targets_to_win=2, max_episode_steps=120)
NAN, INF = float("nan"), float("inf")
# what the quantiser must get right: NaN, the infinities, ties (to even), values out of range, a tiny value
EDGES = (NAN, INF, -INF, 1.5 / 64, -1.5 / 64, 2.5 / 64, 0.5 / 64, 3.0, -7.0, 1e-30, -0.0, 1.0, -1.0)


# ---------------------------------------------------------------- the rules, written out a second time
def ref_quant(a, shift=0.0):
    """one component: fp32(a + shift), NaN -> 0, clamp, times 64 (exact in a double), Python's round (ties to even)"""
    x = np.float32(np.float32(a) + np.float32(shift))
    if x != x:
        return 0
    x = min(max(float(x), -1.0), 1.0)
    return round(x * 64)


class Ref:
    """the world of the issue, as plain ints: state words in the order the device keeps them"""

    def __init__(self, seed, env, targets_to_win=3, max_episode_steps=1000, frame_skip=1, frame_skip_max=None, sticky_num=0,
                 sticky_den=1):
        self.seed, self.env, self.ttw, self.cap = seed, env, targets_to_win, max_episode_steps
        self.k0, self.k1 = frame_skip, frame_skip if frame_skip_max is None else frame_skip_max
        self.sn, self.sd = sticky_num, sticky_den
        self.draws = self.steps = self.ep_steps = self.ep_rew = self.prev = 0
        self.new()

    def draw(self):
        d = hash32(self.seed, self.env, self.draws)
        self.draws += 1
        return d

    @staticmethod
    def place(d):
        return 512 + (d & 0xFFF) % 3072, 512 + ((d >> 12) & 0xFFF) % 3072

    def new(self):
        self.px, self.py = self.place(self.draw())
        self.tx, self.ty = self.place(self.draw())
        self.vx = self.vy = self.got = self.ep_steps = 0

    def cells(self):
        return (abs(self.px - self.tx) + abs(self.py - self.ty)) // 64

    def frame(self, qx, qy):
        self.steps += 1
        self.ep_steps += 1
        d0 = self.cells()
        for ax, q in (("x", qx), ("y", qy)):
            v = min(max(getattr(self, "v" + ax) + q // 8, -64), 64)          # Python's // is the floor
            p = getattr(self, "p" + ax) + v
            if p < 0:
                p, v = 0, 0
            if p > 4095:
                p, v = 4095, 0
            setattr(self, "v" + ax, v)
            setattr(self, "p" + ax, p)
        d1 = self.cells()
        r = d0 - d1
        if d1 == 0:
            r += 10
            self.got += 1
        over = self.got >= self.ttw or self.ep_steps >= self.cap
        if over:
            self.new()
        elif d1 == 0:
            self.tx, self.ty = self.place(self.draw())
        return r, over

    def agent_step(self, a, shift=0.0):
        """the k-draw first, then per game frame the sticky draw before the frame's own draws; the packed previous action"""
        q = (ref_quant(a[0], shift), ref_quant(a[1], shift))
        k = self.k0
        if self.k1 > self.k0:
            k += self.draw() % (self.k1 - self.k0 + 1)
        R, over = 0, False
        for _ in range(k):
            x = q
            if self.sn > 0:
                if self.draw() % self.sd < self.sn:
                    x = self.prev if isinstance(self.prev, tuple) else (0, 0)
                self.prev = x
            r, over = self.frame(*x)
            R += r
            if over:
                self.prev = 0
                break
        self.ep_rew += R
        closed_rew = self.ep_rew
        if over:
            self.ep_rew = 0
        return R, over, closed_rew

    def words(self):
        prev = self.prev if isinstance(self.prev, tuple) else (0, 0)
        return [self.px, self.py, self.vx, self.vy, self.tx, self.ty, self.got, 0, self.draws, self.steps, self.ep_steps,
                self.ep_rew, (prev[0] & 0xFF) | ((prev[1] & 0xFF) << 8), 0, 0, 0]

    def obs(self):
        return np.array([(2 * self.px - 4095) * 2.0 ** -12, (2 * self.py - 4095) * 2.0 ** -12, self.vx * 2.0 ** -6,
                         self.vy * 2.0 ** -6, (self.tx - self.px) * 2.0 ** -12, (self.ty - self.py) * 2.0 ** -12,
                         self.got * 2.0 ** -3, 1.0], dtype=np.float32)


def twin_words(e, ep_rew):
    return [e.px, e.py, e.vx, e.vy, e.tx, e.ty, e.got, 0, e.draws, e.steps, e.ep_steps, ep_rew, e.prev, 0, 0, 0]


# ---------------------------------------------------------------- the action stream of the issue
def steer(e):
    """the brake-distance controller: per axis the speed from which 8 units of braking a frame stop at the target"""
    out = []
    for p, t, v in ((e.px, e.tx, e.vx), (e.py, e.ty, e.vy)):
        err = t - p
        want = np.sign(err) * min(64, int((16 * abs(err)) ** 0.5))
        out.append(float(np.clip((want - v) / 8.0, -1, 1)))
    return out


@functools.lru_cache(maxsize=None)
def host_play(B, n, rules="plain", shift=0.0, seed=5, edges=True):
    """B host twins played for n agent steps, restarted after a done as the Runner does.  Even envs are steered towards their
    targets, odd envs take uniform(-1.5, 1.5) noise, and with ``edges`` every seventh action of an env is a pair of EDGES.
    The twins receive fp32(raw + shift), the Runner's host path; ``acts`` are the raw actions a device pool with
    ``action_shift = shift`` plays.  -> acts (n, B, 2) float32; rew, done (n, B); obs (n + 1, B, 8): row 0 the reset, row
    t + 1 what step t left (the reset observation after a done); words (n, B, 16): the state words after every step; stats
    (n, 2): dones so far and the rewards they closed; the summed event counts.  Computed once per case, left unchanged."""
    rs = np.random.RandomState(1234)
    envs = [PointEnv(seed=seed, env_id=j, **WORLD, **RULES[rules]) for j in range(B)]
    acts = np.zeros((n, B, 2), dtype=np.float32)
    rew, done = np.zeros((n, B), dtype=np.float32), np.zeros((n, B), dtype=np.float32)
    obs, words = np.zeros((n + 1, B, 8), dtype=np.float32), np.zeros((n, B, 16), dtype=np.int64)
    stats, ep_rew = np.zeros((n, 2), dtype=np.int64), [0] * B
    for j, e in enumerate(envs):
        obs[0, j] = e.reset()[0]
    closed = [0, 0]
    for t in range(n):
        for j, e in enumerate(envs):
            want = rs.uniform(-1.5, 1.5, 2) if j % 2 else steer(e)
            if edges and (t + 3 * j) % 7 == 3:
                i = (t // 7 + j) % len(EDGES)
                want = (EDGES[i], EDGES[(i + 5) % len(EDGES)])
            raw = np.asarray(want, dtype=np.float32) - np.float32(shift)
            acts[t, j] = raw
            o, r, d, _ = e.step(raw + np.float32(shift))
            ep_rew[j] += int(r)
            if d:
                closed[0] += 1
                closed[1] += ep_rew[j]
                ep_rew[j] = 0
                o = e.reset()
            rew[t, j], done[t, j], obs[t + 1, j], words[t, j] = r, float(d), o[0], twin_words(e, ep_rew[j])
        stats[t] = closed
    events = {k: sum(e.events[k] for e in envs) for k in envs[0].events}
    out = dict(acts=acts, rew=rew, done=done, obs=obs, words=words, stats=stats, events=events)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---------------------------------------------------------------- surface
def test_surface_and_reset():
    env = PointEnv(seed=3, env_id=1)
    assert env.action_space.shape == (2,) and not hasattr(env.action_space, "n")
    with pytest.raises(RuntimeError):
        env.step((0.0, 0.0))                      # a new env is reset by its caller, like a gym env
    o = env.reset()
    assert o.shape == (1, 8) and o.dtype == np.float32 and env.draws == 2
    assert (env.px, env.py) == Ref.place(hash32(3, 1, 0)) and (env.tx, env.ty) == Ref.place(hash32(3, 1, 1))
    assert (env.vx, env.vy, env.got, env.ep_steps) == (0, 0, 0, 0)
    o2, rew, done, info = env.step(np.array([1.0, -1.0], dtype=np.float32))
    assert o2.shape == (1, 8) and (env.vx, env.vy) == (8, -8) and isinstance(rew, float) and done is False


def test_the_constants_are_the_documented_ones():
    assert (point.P, point.VMAX, point.CELL, point.REACH_BONUS, point.POINT_WORDS, point.OBS) == (4096, 64, 64, 10, 16, 8)
    assert point.RULE_KEYS == ("frame_skip_max",) and point.ACTION_SIZE == 2
    assert point.DevicePointPool.frame_shape == (1, 8) and point.DevicePointPool.float_actions is True
    assert point.DevicePointPool.n_act == 2


def test_the_factory_pickles_and_sits_behind_a_sequential_environment():
    from a2c_amd import preprocessing
    from a2c_amd.runner import SequentialEnvironment
    f = pickle.loads(pickle.dumps(PointFactory(env_id=4, seed=2, targets_to_win=1)))
    env = SequentialEnvironment("Point-host", preprocessing.null_prep, seed=2, env_fn=f)
    assert env.is_discrete is False and env.n == 2 and env.raw_shape == (1, 8)
    assert isinstance(env.env, PointEnv) and env.env.env_id == 4


# ---------------------------------------------------------------- the quantiser
def test_quantiser_edge_values():
    want = {NAN: 0, INF: 64, -INF: -64, 1.5 / 64: 2, -1.5 / 64: -2, 2.5 / 64: 2, -2.5 / 64: -2, 0.5 / 64: 0, 3.5 / 64: 4,
            3.0: 64, -7.0: -64, 1e-30: 0, -1e-30: 0, 0.0: 0, -0.0: 0, 1.0: 64, -1.0: -64, 63.4 / 64: 63, 0.124: 8, 0.126: 8}
    for a, q in want.items():
        assert int(quantise(a)) == q == ref_quant(a), a
    shifted = {0.25: 48, 0.6: 64, -0.5: 0, 1e-30: 32, NAN: 0, -INF: -64, -1.5: -64, 1.5 / 64 - 0.5: 2, 2.0 ** -25: 32,
               -0.5 + 2.5 / 64: 2}
    for a, q in shifted.items():
        assert int(quantise(a, 0.5)) == q == ref_quant(a, 0.5), a
    # arrays, and every fp32 in a sweep across the range and its ties against the scalar statement
    a = np.concatenate([np.linspace(-1.25, 1.25, 4001), (np.arange(-130, 131) + 0.5) / 64, np.array(EDGES)]).astype(np.float32)
    for s in (0.0, 0.5):
        q = quantise(a, s)
        assert q.dtype == np.int32 and q.shape == a.shape and q.min() == -64 and q.max() == 64
        assert q.tolist() == [ref_quant(x, s) for x in a]


def test_the_packed_pair():
    for qx in (-64, -9, -8, -1, 0, 1, 7, 8, 64):
        for qy in (-64, -1, 0, 3, 64):
            assert point.unpack(point.pack(qx, qy)) == (qx, qy)
    assert point.pack(0, 0) == 0 and point.unpack(0) == (0, 0)


# ---------------------------------------------------------------- the twin against the loop written out above
@pytest.mark.parametrize("rules", list(RULES))
def test_point_env_equals_the_written_out_loop(rules):
    B, n = 7, 300
    h = host_play(B, n, rules)
    refs = [Ref(5, j, **WORLD, **RULES[rules]) for j in range(B)]
    assert all(np.array_equal(r.obs(), h["obs"][0, j]) for j, r in enumerate(refs))
    closed = [0, 0]
    for t in range(n):
        for j, r in enumerate(refs):
            R, over, closed_rew = r.agent_step(h["acts"][t, j])
            if over:
                closed[0] += 1
                closed[1] += closed_rew
            assert (float(R), float(over)) == (h["rew"][t, j], h["done"][t, j]), (t, j)
            assert r.words() == h["words"][t, j].tolist(), (t, j)
            assert np.array_equal(r.obs(), h["obs"][t + 1, j]), (t, j)
        assert closed == h["stats"][t].tolist(), t
    assert np.abs(h["rew"]).max() <= 8 * 3 + 10 and (h["rew"] == np.round(h["rew"])).all()


def test_the_shifted_stream_is_the_same_world():
    """raw actions with action_shift = 0.5: the twin receives fp32(raw + 0.5), what the loop quantises with shift 0.5"""
    B, n = 3, 120
    h = host_play(B, n, "repeat", 0.5)
    refs = [Ref(5, j, **WORLD, **REPEAT) for j in range(B)]
    for t in range(n):
        for j, r in enumerate(refs):
            R, over, _ = r.agent_step(h["acts"][t, j], 0.5)
            assert (float(R), float(over)) == (h["rew"][t, j], h["done"][t, j]) and r.words() == h["words"][t, j].tolist()


@pytest.mark.parametrize("rules,edges", [("plain", False), ("plain", True), ("repeat", False), ("repeat", True)])
def test_the_stream_shows_every_rule_at_work(rules, edges):
    """seven envs, targets_to_win = 2, max_episode_steps = 120, 300 steps: even envs steered, odd envs noise"""
    ev = host_play(7, 300, rules, edges=edges)["events"]
    print(f"point stream {rules} edges={edges}: {ev}")
    names = ("wall", "reach", "end_targets", "end_cap") + (("cut", "sticky") if rules == "repeat" else ())
    assert set(ev) == set(names) and all(ev[k] > 0 for k in names), ev


def test_observations_are_exact_fractions():
    h = host_play(7, 300, "plain")
    o = h["obs"].astype(np.float64)
    for col, scale in ((0, 4096), (1, 4096), (2, 64), (3, 64), (4, 4096), (5, 4096), (6, 8)):
        assert np.array_equal(o[..., col] * scale, np.round(o[..., col] * scale))
    assert (o[..., 7] == 1.0).all() and np.abs(o[..., :2]).max() < 1 and np.abs(o[..., 2:4]).max() <= 1


# ---------------------------------------------------------------- bounds
def test_world_bounds_and_hyps():
    assert world_from_hyps({}) == (3, 1000) and world_from_hyps(dict(targets_to_win=8, max_episode_steps=1 << 24)) == (8, 1 << 24)
    assert world_from_hyps(dict(targets_to_win=None)) == (3, 1000)
    for bad in (dict(targets_to_win=0), dict(targets_to_win=9), dict(max_episode_steps=0), dict(max_episode_steps=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            world_from_hyps(bad)
        with pytest.raises(ValueError):
            point.check_world(**bad)
        with pytest.raises(ValueError):
            PointEnv(**bad)
        with pytest.raises(ValueError):
            point.DevicePointPool(2, "cpu", **bad)            # refused before anything is allocated
    for bad in (dict(frame_skip=0), dict(frame_skip=9), dict(frame_skip=3, frame_skip_max=2), dict(frame_skip_max=9),
                dict(sticky_num=2, sticky_den=1), dict(sticky_num=-1), dict(sticky_den=0), dict(sticky_den=(1 << 16) + 1)):
        with pytest.raises(ValueError):
            point.check_world(**bad)
        with pytest.raises(ValueError):
            PointEnv(**bad)
        with pytest.raises(ValueError):
            point.DevicePointPool(2, "cpu", **bad)
    with pytest.raises(ValueError):
        point.DevicePointPool(0, "cpu")
    with pytest.raises(ValueError):
        point.DevicePointPool(2, "cpu", env_id0=-1)
    with pytest.raises(TypeError):
        PointEnv(episodic_life=True)                          # keys of the Breakout worlds: not keywords here
    with pytest.raises(TypeError):
        point.DevicePointPool(2, "cpu", clip_rewards=True)
    assert point.rules_from_hyps(dict(frame_skip=2, frame_skip_max=4)) == dict(frame_skip_max=4)
    assert point.rules_from_hyps({}) == dict(frame_skip_max=1)
    for bad in (dict(episodic_life=True), dict(clip_rewards=1), dict(frame_skip=4, frame_skip_max=2)):
        with pytest.raises(ValueError):
            point.rules_from_hyps(bad)


@pytest.mark.parametrize("env_type,kw", [
    ("Point-device", dict(episodic_life=True)), ("Point-host", dict(clip_rewards=True)), ("Point-host", dict(frame_skip_max=9)),
    ("Point-device", dict(frame_skip=4, frame_skip_max=2)), ("Point-device", dict(model="A3CModel")),
    ("Point-host", dict(model="ConvModel")), ("Point-host", dict(model="GRUModel")), ("Point-device", dict(is_discrete=True)),
    ("Point-host", dict(model="GRUFCModel", is_discrete=True)), ("Point-host", dict(env_pool="process")),
    ("Point-host", dict(env_pool="thread")), ("Point-host", dict(eval_pool="device"))])
def test_train_refuses_before_the_device(env_type, kw, tmp_path, monkeypatch):
    import torch
    from a2c_amd.training import train

    def no_device(*a, **k):
        raise AssertionError("train() touched the device")
    monkeypatch.setattr(torch.Tensor, "cuda", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    hyps = dict(dict(exp_name="point", main_path=str(tmp_path), model="FCModel", env_type=env_type, n_envs=2, n_rollouts=2,
                     n_tsteps=2, n_frame_stack=2, max_tsteps=1e9, seed=1, h_size=16), **kw)
    with pytest.raises(ValueError):
        train(None, hyps, verbose=False, max_epochs=1)
    assert not list(tmp_path.iterdir()), "nothing was written either"


def test_host_world_action_hook_keeps_the_discrete_twins():
    """HostWorld._action: the default is int(action) mod N_ACTIONS, what advance() computed in line before"""
    from a2c_amd.breakout import BreakoutEnv
    from a2c_amd.pong import PongEnv
    for env, n in ((PongEnv(), 3), (BreakoutEnv(), 4)):
        assert [env._action(a) for a in (-4, -1, 0, 1, 5, np.int64(7))] == [a % n for a in (-4, -1, 0, 1, 5, 7)]
