"""Pendulum on the host (no GPU needed): ``a2c_amd.pendulum.PendulumEnv`` against an agent-step loop
written out here, value for value; the action quantiser on its edge values; ``sincos`` and one game frame against float64
within the bound DESIGN.md section 6l derives (``derived_bounds`` restates the derivation as arithmetic; the measured worst
is printed beside it); the reward range; the bounds of the world, pool, twin and ``train()`` keys.  The device worlds are
compared with this host twin in test_gpu_pendulum.py, which plays the streams built here."""
import functools
import math
import pickle

import numpy as np
import pytest

from a2c_amd import pendulum
from a2c_amd.pendulum import PendulumEnv, PendulumFactory, quantise, world_from_hyps
from a2c_amd.worlds import hash32

PLAIN = dict()
REPEAT = dict(frame_skip=2, frame_skip_max=4, sticky_num=1, sticky_den=4)          # (2, 4, sticky 1/4)
RULES = {"plain": PLAIN, "repeat": REPEAT}
CAP = 7                                                                             # closes happen, all envs together
NAN, INF = float("nan"), float("inf")
# what the quantiser must get right: NaN, the infinities, ties (to even, both parities), values out of range, a tiny value
EDGES = (NAN, INF, -INF, 1.5 / 32, -1.5 / 32, 2.5 / 32, 0.5 / 32, 3.0, -7.0, 1e-30, -0.0, 2.0, -2.0)
ONE, PI, HALF_PI, TWO_PI, VMAX = 1 << 20, 3294199, 1647099, 6588398, 8 << 20


# ---------------------------------------------------------------- the rules, written out a second time
def ref_quant(a, shift=0.0):
    """fp32(a + shift), NaN -> 0, clamp to +-2, times 32 (exact in a double), Python's round (ties to even)"""
    x = np.float32(np.float32(a) + np.float32(shift))
    if x != x:
        return 0
    return round(min(max(float(x), -2.0), 2.0) * 32)


def ref_sincos(th):
    m = lambda a, b: (a * b) >> 20
    neg = False
    x = th
    if th > 1647099:
        x, neg = 3294199 - th, True
    if th < -1647099:
        x, neg = -3294199 - th, True
    x2 = m(x, x)
    p = ONE - m(x2, 9533)
    p = ONE - m(m(x2, 14564), p)
    p = ONE - m(m(x2, 24966), p)
    p = ONE - m(m(x2, 52429), p)
    p = ONE - m(m(x2, 174763), p)
    s = m(x, p)
    p = ONE - m(x2, 7944)
    p = ONE - m(m(x2, 11651), p)
    p = ONE - m(m(x2, 18725), p)
    p = ONE - m(m(x2, 34953), p)
    p = ONE - m(m(x2, 87381), p)
    p = ONE - m(m(x2, 524288), p)
    return s, -p if neg else p


class Ref:
    """the world of the issue, as plain ints: state words in the order the device keeps them; rewards in units of 2^-8"""

    def __init__(self, seed, env, max_episode_steps=200, frame_skip=1, frame_skip_max=None, sticky_num=0, sticky_den=1):
        self.seed, self.env, self.cap = seed, env, max_episode_steps
        self.k0, self.k1 = frame_skip, frame_skip if frame_skip_max is None else frame_skip_max
        self.sn, self.sd = sticky_num, sticky_den
        self.draws = self.steps = self.ep_steps = self.ep_rew = self.prev = 0
        self.new()

    def draw(self):
        d = hash32(self.seed, self.env, self.draws)
        self.draws += 1
        return d

    def new(self):
        self.th = self.draw() % 6588398 - 3294199
        self.thd = self.draw() % 2097153 - 1048576
        self.ep_steps = 0

    def frame(self, q):
        m = lambda a, b: (a * b) >> 20
        self.steps += 1
        self.ep_steps += 1
        u = q * 32768
        cost = m(self.th, self.th) + m(104858, m(self.thd, self.thd)) + m(1049, m(u, u))
        s, _ = ref_sincos(self.th)
        self.thd = min(max(self.thd + m(786432, s) + m(157286, u), -VMAX), VMAX)
        self.th += m(52429, self.thd)
        if self.th >= 3294199:
            self.th -= 6588398
        elif self.th < -3294199:
            self.th += 6588398
        over = self.ep_steps >= self.cap
        if over:
            self.new()
        return -(cost >> 12), over

    def agent_step(self, a, shift=0.0):
        """the k-draw first, then per game frame the sticky draw before the frame; -> (R, over, closed_rew) in units of 2^-8"""
        q = ref_quant(a, shift)
        k = self.k0
        if self.k1 > self.k0:
            k += self.draw() % (self.k1 - self.k0 + 1)
        R, over = 0, False
        for _ in range(k):
            x = q
            if self.sn > 0:
                if self.draw() % self.sd < self.sn:
                    x = self.prev
                self.prev = x
            r, over = self.frame(x)
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
        return [self.th, self.thd, 0, 0, self.draws, self.steps, self.ep_steps, self.ep_rew, self.prev, 0, 0, 0]

    def obs(self):
        s, c = ref_sincos(self.th)
        return np.array([c * 2.0 ** -20, s * 2.0 ** -20, self.thd * 2.0 ** -20, 0.0], dtype=np.float32)


def twin_words(e, ep_rew):
    return [e.th, e.thd, 0, 0, e.draws, e.steps, e.ep_steps, ep_rew, e.prev, 0, 0, 0]


# ---------------------------------------------------------------- the action streams
class _Recorded(PendulumEnv):
    """a twin that keeps every game frame: (th, thd, q) before, (th, thd) after, the reward in units of 2^-8"""
    frames = None

    def _frame(self, q):
        th, thd = self.th, self.thd
        rew, done = super()._frame(q)
        if self.frames is not None:
            self.frames.append((th, thd, q, self.th, self.thd, int(rew * 256)))
        return rew, done


@functools.lru_cache(maxsize=None)
def host_play(B, n, rules="plain", shift=0.0, cap=CAP, seed=5, edges=True, record=False):
    """B host twins played for n agent steps, restarted after a done as the Runner does.  Even envs pump energy in (a torque
    with the sign of the speed, jittered), odd envs take uniform(-2.5, 2.5) noise, and with ``edges`` every seventh action of an
    env is one of EDGES.  The twins receive fp32(raw + shift), the Runner's host path; ``acts`` are the raw actions a device
    pool with ``action_shift = shift`` plays.  -> acts (n, B) float32; rew, done (n, B); obs (n + 1, B, 4): row 0 the reset,
    row t + 1 what step t left (the reset observation after a done); words (n, B, 12): the state words after every step;
    stats (n, 2): dones so far and the sum of the episode rewards they closed, each FLOORED to whole units; sums: the exact
    episode rewards closed, in units of 2^-8; the summed event counts; with ``record`` the game frames played.  Computed once
    per case, left unchanged."""
    rs = np.random.RandomState(1234)
    frames = [] if record else None
    envs = [_Recorded(seed=seed, env_id=j, max_episode_steps=cap, **RULES[rules]) for j in range(B)]
    for e in envs:
        e.frames = frames
    acts = np.zeros((n, B), dtype=np.float32)
    rew, done = np.zeros((n, B), dtype=np.float32), np.zeros((n, B), dtype=np.float32)
    obs, words = np.zeros((n + 1, B, 4), dtype=np.float32), np.zeros((n, B, 12), dtype=np.int64)
    stats, ep_rew, sums = np.zeros((n, 2), dtype=np.int64), [0] * B, []
    for j, e in enumerate(envs):
        obs[0, j] = e.reset()[0]
    closed = [0, 0]
    for t in range(n):
        for j, e in enumerate(envs):
            want = rs.uniform(-2.5, 2.5) if j % 2 else (2.0 if e.thd >= 0 else -2.0) * rs.uniform(0.5, 1.2)
            if edges and (t + 3 * j) % 7 == 3:
                want = EDGES[(t // 7 + j) % len(EDGES)]
            raw = np.float32(want) - np.float32(shift)
            acts[t, j] = raw
            o, r, d, _ = e.step(np.float32(raw + np.float32(shift)))
            assert r * 256 == int(r * 256) and -8 * 4166 <= r * 256 <= 0
            ep_rew[j] += int(r * 256)
            if d:
                closed[0] += 1
                closed[1] += ep_rew[j] >> 8              # the floor to whole units
                sums.append(ep_rew[j])
                ep_rew[j] = 0
                o = e.reset()
            rew[t, j], done[t, j], obs[t + 1, j], words[t, j] = r, float(d), o[0], twin_words(e, ep_rew[j])
        stats[t] = closed
    events = {k: sum(e.events[k] for e in envs) for k in envs[0].events}
    out = dict(acts=acts, rew=rew, done=done, obs=obs, words=words, stats=stats, events=events, sums=tuple(sums))
    if record:
        out["frames"] = np.array(frames, dtype=np.int64)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---------------------------------------------------------------- the bound of DESIGN.md section 6l, as arithmetic
def _series_err(ks, zmax):
    """the error interval (units of 2^-20, computed - exact) of the nested series p after its levels, for x^2 <= zmax: per
    level t = mul(x2, r) is off by the floor of x2 (over k), the rounding of the ratio (times x^2) and its own floor; the
    product mul(t, p) by t's error (p <= 1), p's error (times t <= zmax / k) and its own floor; p = ONE - product"""
    lo = hi = 0.0
    tiny = 1e-5                                   # the products of two errors, over 2^20
    for k in ks:
        dc = round(ONE / k) - ONE / k
        t_lo, t_hi = -1.0 / k + min(0.0, zmax * dc) - 1.0 - tiny, max(0.0, zmax * dc) + tiny
        m_lo = t_lo + (zmax / k) * min(0.0, lo) - 1.0 - tiny
        m_hi = t_hi + (zmax / k) * max(0.0, hi) + tiny
        lo, hi = -m_hi, -m_lo
    return lo, hi


def derived_bounds():
    """-> the worst one-frame deviations from a float64 Euler step DESIGN.md section 6l derives: sin, cos, th, thd in units of
    2^-20 and the frame reward in units of 2^-8"""
    xm = (HALF_PI + 1) / ONE                       # |x| after the reflection: PI - (HALF_PI + 1) < HALF_PI + 1
    z = xm * xm
    d_pi = abs(PI - math.pi * ONE)                 # the reflection and the wrap use the rounded PI
    trunc_s = xm ** 13 / math.factorial(13) * ONE
    trunc_c = xm ** 14 / math.factorial(14) * ONE
    e_s = xm * max(abs(v) for v in _series_err(pendulum.SIN_K, z)) + 1.0 + trunc_s + d_pi
    e_c = max(abs(v) for v in _series_err(pendulum.COS_K, z)) + trunc_c + d_pi
    # thd + mul(C075, s) + mul(C015, u): C075 is exact; |u| <= 2; two floors; the clamp does not stretch
    e_thd = 0.75 * e_s + 1.0 + 2.0 * abs(157286 - 0.15 * ONE) + 1.0
    # th + mul(DT, thd'): |thd'| <= 8; one floor; a wrap takes 2 PI (rounded) off
    e_th = 0.05 * e_thd + 8.0 * abs(52429 - 0.05 * ONE) + 1.0 + 2.0 * d_pi
    # the cost: three products floored, 0.1 and 0.001 rounded (times thd^2 <= 64 and u^2 <= 4); then >> 12, one more floor
    e_cost = (1.0 + 0.1 + 1.0 + 0.001 + 1.0) + 64.0 * abs(104858 - 0.1 * ONE) + 4.0 * abs(1049 - 0.001 * ONE)
    return dict(sin=e_s, cos=e_c, th=e_th, thd=e_thd, rew=1.0 + e_cost / 4096.0)


# what DESIGN.md section 6l quotes (the derivation above, rounded up)
QUOTED = dict(sin=5.31, cos=4.27, th=3.63, thd=6.79, rew=1.0075)


def test_the_derived_bound_is_the_quoted_one():
    b = derived_bounds()
    print("pendulum derived bounds:", {k: round(v, 4) for k, v in b.items()})
    for k, v in QUOTED.items():
        assert b[k] <= v < b[k] * 1.01 + 1e-4, (k, b[k], v)


# ---------------------------------------------------------------- surface
def test_surface_and_reset():
    env = PendulumEnv(seed=3, env_id=1)
    assert env.action_space.shape == (1,) and not hasattr(env.action_space, "n")
    with pytest.raises(RuntimeError):
        env.step(0.0)                             # a new env is reset by its caller, like a gym env
    o = env.reset()
    assert o.shape == (1, 4) and o.dtype == np.float32 and env.draws == 2
    assert env.th == hash32(3, 1, 0) % TWO_PI - PI and env.thd == hash32(3, 1, 1) % (2 * ONE + 1) - ONE
    assert -PI <= env.th < PI and -ONE <= env.thd <= ONE and env.ep_steps == 0
    thd = env.thd
    o2, rew, done, info = env.step(np.array([2.0], dtype=np.float32))
    assert o2.shape == (1, 4) and isinstance(rew, float) and rew <= 0 and done is False and env.thd != thd
    assert env.max_episode_steps == 200


def test_the_constants_are_the_documented_ones():
    q = lambda v: int(round(v * ONE))
    assert (pendulum.PI, pendulum.HALF_PI, pendulum.TWO_PI) == (q(math.pi), q(math.pi / 2), 2 * q(math.pi)) == (PI, HALF_PI, TWO_PI)
    assert (pendulum.C075, pendulum.C015, pendulum.DT, pendulum.C01, pendulum.C0001) == (q(.75), q(.15), q(.05), q(.1), q(.001))
    assert (pendulum.C075, pendulum.C015, pendulum.DT, pendulum.C01, pendulum.C0001) == (786432, 157286, 52429, 104858, 1049)
    assert pendulum.VMAX == 8 * ONE and pendulum.ONE == ONE and (pendulum.PENDULUM_WORDS, pendulum.OBS) == (12, 4)
    assert pendulum.SIN_R == (9533, 14564, 24966, 52429, 174763) and pendulum.COS_R == (7944, 11651, 18725, 34953, 87381, 524288)
    assert pendulum.RULE_KEYS == ("frame_skip_max",) and pendulum.ACTION_SIZE == 1
    P = pendulum.DevicePendulumPool
    assert P.frame_shape == (1, 4) and P.float_actions is True and P.n_act == 1


def test_the_factory_pickles_and_sits_behind_a_sequential_environment():
    from a2c_amd import preprocessing
    from a2c_amd.runner import SequentialEnvironment
    f = pickle.loads(pickle.dumps(PendulumFactory(env_id=4, seed=2, max_episode_steps=9)))
    env = SequentialEnvironment("Pendulum-host", preprocessing.null_prep, seed=2, env_fn=f)
    assert env.is_discrete is False and env.n == 1 and env.raw_shape == (1, 4)
    assert isinstance(env.env, PendulumEnv) and env.env.env_id == 4 and env.env.max_episode_steps == 9


# ---------------------------------------------------------------- the quantiser
def test_quantiser_edge_values():
    want = {NAN: 0, INF: 64, -INF: -64, 1.5 / 32: 2, -1.5 / 32: -2, 2.5 / 32: 2, -2.5 / 32: -2, 0.5 / 32: 0, 3.5 / 32: 4,
            3.0: 64, -7.0: -64, 1e-30: 0, -1e-30: 0, 0.0: 0, -0.0: 0, 2.0: 64, -2.0: -64, 63.4 / 32: 63, 1.0: 32, 0.249: 8,
            0.251: 8, 63.5 / 32: 64, 62.5 / 32: 62}
    for a, q in want.items():
        assert int(quantise(a)) == q == ref_quant(a), a
    shifted = {0.25: 24, 1.6: 64, -0.5: 0, 1e-30: 16, NAN: 0, -INF: -64, -2.6: -64, 1.5 / 32 - 0.5: 2, 2.0 ** -25: 16,
               -0.5 + 2.5 / 32: 2, INF: 64}
    for a, q in shifted.items():
        assert int(quantise(a, 0.5)) == q == ref_quant(a, 0.5), a
    # arrays, and every fp32 in a sweep across the range and its ties against the scalar statement
    a = np.concatenate([np.linspace(-2.5, 2.5, 4001), (np.arange(-130, 131) + 0.5) / 32, np.array(EDGES)]).astype(np.float32)
    for s in (0.0, 0.5):
        q = quantise(a, s)
        assert q.dtype == np.int32 and q.shape == a.shape and q.min() == -64 and q.max() == 64
        assert q.tolist() == [ref_quant(x, s) for x in a]
    env = PendulumEnv()
    assert [env._action(v) for v in (NAN, 3.0, np.float32(-1.5 / 32), [0.5], np.array([-INF]))] == [0, 64, -2, 16, -64]


# ---------------------------------------------------------------- the twin against the loop written out above
@pytest.mark.parametrize("rules", list(RULES))
def test_pendulum_env_equals_the_written_out_loop(rules):
    B, n = 7, 300
    h = host_play(B, n, rules)
    refs = [Ref(5, j, CAP, **RULES[rules]) for j in range(B)]
    assert all(np.array_equal(r.obs(), h["obs"][0, j]) for j, r in enumerate(refs))
    closed, sums = [0, 0], []
    for t in range(n):
        for j, r in enumerate(refs):
            R, over, closed_rew = r.agent_step(h["acts"][t, j])
            if over:
                closed[0] += 1
                closed[1] += closed_rew >> 8
                sums.append(closed_rew)
            assert (np.float32(R / 256), float(over)) == (h["rew"][t, j], h["done"][t, j]), (t, j)
            assert r.words() == h["words"][t, j].tolist(), (t, j)
            assert np.array_equal(r.obs(), h["obs"][t + 1, j]), (t, j)
        assert closed == h["stats"][t].tolist(), t
    assert tuple(sums) == h["sums"] and closed[0] >= B
    # the floored whole-unit sum: each closed episode's total floored, -833.6 -> -834
    assert closed[1] == sum(math.floor(s / 256) for s in sums) and any(s % 256 for s in sums)
    assert closed[1] < sum(sums) / 256 < closed[1] + len(sums)
    ev = h["events"]
    assert ev["end_cap"] == closed[0] and all(ev[k] > 0 for k in (("cut", "sticky") if rules == "repeat" else ())), ev


def test_the_shifted_stream_is_the_same_world():
    """raw actions with action_shift = 0.5: the twin receives fp32(raw + 0.5), what the loop quantises with shift 0.5"""
    B, n = 3, 120
    h = host_play(B, n, "repeat", 0.5)
    refs = [Ref(5, j, CAP, **REPEAT) for j in range(B)]
    for t in range(n):
        for j, r in enumerate(refs):
            R, over, _ = r.agent_step(h["acts"][t, j], 0.5)
            assert (np.float32(R / 256), float(over)) == (h["rew"][t, j], h["done"][t, j]) and r.words() == h["words"][t, j].tolist()


def test_observations_are_exact_fractions():
    h = host_play(7, 300, "plain")
    o = h["obs"].astype(np.float64) * 2 ** 20
    assert np.array_equal(o, np.round(o)) and (o[..., 3] == 0).all()
    assert np.abs(o[..., :2]).max() <= ONE + 4 and np.abs(o[..., 2]).max() <= VMAX
    assert np.abs(o[..., 0] ** 2 + o[..., 1] ** 2 - 2.0 ** 40).max() < 2.0 ** 24      # cos^2 + sin^2 = 1 within 8 units


# ---------------------------------------------------------------- against float64
def test_sincos_against_float64():
    b = derived_bounds()
    ths = sorted(set(list(range(-PI, PI, 997)) + [s * v + d for s in (-1, 1) for v in (PI, HALF_PI) for d in (-1, 0, 1)
                                                  if -PI <= s * v + d < PI] + [0, 1, -1, PI - 1, -PI]))
    assert len(ths) > 6000
    worst = [0.0, 0.0]
    for th in ths:
        s, c = pendulum.sincos(th)
        assert (s, c) == ref_sincos(th)
        worst[0] = max(worst[0], abs(s - math.sin(th / ONE) * ONE))
        worst[1] = max(worst[1], abs(c - math.cos(th / ONE) * ONE))
    print(f"pendulum sincos: worst sin {worst[0]:.3f} (bound {b['sin']:.3f}), cos {worst[1]:.3f} (bound {b['cos']:.3f}) units "
          "of 2^-20")
    assert worst[0] <= b["sin"] and worst[1] <= b["cos"]


def test_one_frame_against_a_float64_step():
    """every game frame of 64 twins over 700 agent steps on the (2, 4, 1/4) world with max_episode_steps = 60, more than
    100 000 frames, the speed clamp and both wraps among them, plus 20 000 states drawn over the whole state space and the
    edges: th, thd and the reward of the frame against the float64 Euler step from the same state, th modulo 2 pi"""
    b = derived_bounds()
    h = host_play(64, 700, "repeat", 0.0, 60, 11, True, True)
    ev = h["events"]
    print(f"pendulum frames: {len(h['frames'])} played, events {ev}")
    assert set(ev) == {"wrap_pos", "wrap_neg", "clamp", "end_cap", "cut", "sticky"} and all(v > 0 for v in ev.values()), ev
    rs = np.random.RandomState(7)
    n = 20000
    extra = np.stack([rs.randint(-PI, PI, n), rs.randint(-VMAX, VMAX + 1, n), rs.randint(-64, 65, n)], 1).tolist()
    extra += [[s * v + d, w, q] for s in (-1, 1) for v in (PI, HALF_PI) for d in (-1, 0, 1) for w in (-VMAX, 0, VMAX)
              for q in (-64, 0, 64) if -PI <= s * v + d < PI]
    extra += [[0, 0, 0], [PI - 1, VMAX, 64], [-PI, -VMAX, -64]]
    rows = [(th, thd, q) + pendulum.physics(th, thd, q)[:3] for th, thd, q in extra]
    rows = np.array([r[:5] + (-(r[5] >> 12),) for r in rows], dtype=np.int64)
    f = np.concatenate([h["frames"], rows]).astype(np.float64)
    assert len(f) >= 100000 + n
    assert f[:, 5].min() >= -4166 and f[:, 5].max() <= 0, "every frame reward lies in -4166 .. 0"
    assert (np.abs(f[:, 4]) == VMAX).any() and (f[:, 3] >= -PI).all() and (f[:, 3] < PI).all()
    th, thd, u = f[:, 0] / ONE, f[:, 1] / ONE, f[:, 2] / 32
    cost = th * th + 0.1 * thd * thd + 0.001 * u * u
    nthd = np.clip(thd + 0.75 * np.sin(th) + 0.15 * u, -8.0, 8.0)
    nth = th + 0.05 * nthd
    d_th = np.abs((f[:, 3] / ONE - nth + math.pi) % (2 * math.pi) - math.pi) * ONE
    d_thd = np.abs(f[:, 4] / ONE - nthd) * ONE
    d_rew = np.abs(f[:, 5] + cost * 256)
    print(f"pendulum one frame, {len(f)} states: worst th {d_th.max():.3f} (bound {b['th']:.3f}), thd {d_thd.max():.3f} "
          f"(bound {b['thd']:.3f}) units of 2^-20; reward {d_rew.max():.5f} (bound {b['rew']:.5f}) units of 2^-8")
    assert d_th.max() <= b["th"] and d_thd.max() <= b["thd"] and d_rew.max() <= b["rew"]
    assert -4166 == -(pendulum.physics(-PI, VMAX, 64)[2] >> 12), "the worst frame is worth -4166"


def test_a_uniform_random_policy_scores_like_the_prototype():
    """200 episodes of 200 frames under uniform(-2, 2) torques: the issue's prototype averaged -1225 (min -1818, max -747)"""
    rs = np.random.RandomState(3)
    tot = []
    for j in range(40):
        e = PendulumEnv(seed=9, env_id=j)
        e.reset()
        R, done = 0.0, False
        while not done:
            _, r, done, _ = e.step(rs.uniform(-2, 2))
            R += r
        tot.append(R)
    print(f"pendulum uniform-random policy, 40 episodes: mean {np.mean(tot):.1f} min {min(tot):.1f} max {max(tot):.1f}")
    assert e.steps == 200 and -2000 < min(tot) and max(tot) < -500 and -1500 < np.mean(tot) < -950


# ---------------------------------------------------------------- bounds
def test_world_bounds_and_hyps():
    assert world_from_hyps({}) == (200,) and world_from_hyps(dict(max_episode_steps=1 << 16)) == (1 << 16,)
    assert world_from_hyps(dict(max_episode_steps=None)) == (200,)
    for bad in (dict(max_episode_steps=0), dict(max_episode_steps=-3), dict(max_episode_steps=(1 << 16) + 1)):
        with pytest.raises(ValueError):
            world_from_hyps(bad)
        with pytest.raises(ValueError):
            pendulum.check_world(**bad)
        with pytest.raises(ValueError):
            PendulumEnv(**bad)
        with pytest.raises(ValueError):
            pendulum.DevicePendulumPool(2, "cpu", **bad)            # refused before anything is allocated
    for bad in (dict(frame_skip=0), dict(frame_skip=9), dict(frame_skip=3, frame_skip_max=2), dict(frame_skip_max=9),
                dict(sticky_num=2, sticky_den=1), dict(sticky_num=-1), dict(sticky_den=0), dict(sticky_den=(1 << 16) + 1)):
        with pytest.raises(ValueError):
            pendulum.check_world(**bad)
        with pytest.raises(ValueError):
            PendulumEnv(**bad)
        with pytest.raises(ValueError):
            pendulum.DevicePendulumPool(2, "cpu", **bad)
    with pytest.raises(ValueError):
        pendulum.DevicePendulumPool(0, "cpu")
    with pytest.raises(ValueError):
        pendulum.DevicePendulumPool(2, "cpu", env_id0=-1)
    with pytest.raises(TypeError):
        PendulumEnv(episodic_life=True)                          # keys of the Breakout worlds: not keywords here
    with pytest.raises(TypeError):
        pendulum.DevicePendulumPool(2, "cpu", clip_rewards=True)
    assert pendulum.rules_from_hyps(dict(frame_skip=2, frame_skip_max=4)) == dict(frame_skip_max=4)
    assert pendulum.rules_from_hyps({}) == dict(frame_skip_max=1)
    for bad in (dict(episodic_life=True), dict(clip_rewards=1), dict(frame_skip=4, frame_skip_max=2)):
        with pytest.raises(ValueError):
            pendulum.rules_from_hyps(bad)


REFUSALS = [
    ("Pendulum-device", dict(episodic_life=True)), ("Pendulum-host", dict(clip_rewards=True)),
    ("Pendulum-host", dict(frame_skip_max=9)), ("Pendulum-device", dict(frame_skip=4, frame_skip_max=2)),
    ("Pendulum-device", dict(model="A3CModel")),
    ("Pendulum-host", dict(model="ConvModel")), ("Pendulum-host", dict(model="GRUModel")),
    ("Pendulum-device", dict(is_discrete=True)), ("Pendulum-host", dict(model="GRUFCModel", is_discrete=True)),
    ("Pendulum-host", dict(env_pool="process")), ("Pendulum-host", dict(env_pool="thread")),
    ("Pendulum-host", dict(eval_pool="device"))]


@pytest.mark.parametrize("env_type,kw", REFUSALS)
def test_train_refuses_before_the_device(env_type, kw, tmp_path, monkeypatch):
    import torch
    from a2c_amd.training import train

    def no_device(*a, **k):
        raise AssertionError("train() touched the device")
    monkeypatch.setattr(torch.Tensor, "cuda", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    hyps = dict(dict(exp_name="pendulum", main_path=str(tmp_path), model="FCModel", env_type=env_type, n_envs=2, n_rollouts=2,
                     n_tsteps=2, n_frame_stack=2, max_tsteps=1e9, seed=1, h_size=16), **kw)
    with pytest.raises(ValueError):
        train(None, hyps, verbose=False, max_epochs=1)
    assert not list(tmp_path.iterdir()), "nothing was written either"
