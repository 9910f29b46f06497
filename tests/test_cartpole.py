"""CartPole on the host (no GPU needed): ``a2c_amd.cartpole.CartPoleEnv``: determinism and the reset
draws; action streams that end episodes by every cause; one game frame against one float64 Euler step of the same equations,
within the bound section 6k derives from the formats; the agent step against the plain world stepped frame by frame; the
argument checks of the three entry points (no launch, so no GPU); the bounds of the world, pool, twin and ``train()`` keys;
header, bindings and generated ops.  The device worlds are compared with this host twin in test_gpu_cartpole.py, which plays
the streams built here."""
import ctypes
import functools
import math
import os
import pickle
import re

import numpy as np
import pytest

from a2c_amd import cartpole
from a2c_amd.cartpole import CartPoleEnv, CartPoleFactory, world_from_hyps
from a2c_amd.worlds import hash32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = dict()
REPEAT = dict(frame_skip=2, frame_skip_max=4, sticky_num=1, sticky_den=4)          # (2, 4, sticky 1/4)
RULES = {"plain": PLAIN, "repeat": REPEAT}
SEED = 5
U = cartpole.UNIT

# The scripted feedback controller: push right when K . (x, x_dot, theta, theta_dot) + BIAS > 0, on the state INTS.  It holds
# the pole at a lean of about BIAS / K[2] units to the right, which takes a steady push to the right: the cart drifts to the
# x limit in 114 .. 140 frames (seed 5, env ids 0 .. 139; found on the CPU), the pole never reaching 12 degrees.
K, BIAS = (0, 0, 4, 1), -400000


def controller(e):
    return 1 if K[0] * e.x + K[1] * e.xd + K[2] * e.th + K[3] * e.thd + BIAS > 0 else 0


def play(env, policy, limit=2000):
    """one episode -> frames played"""
    env.reset()
    for n in range(1, limit + 1):
        if env.step(policy(env, n))[2]:
            return n
    raise AssertionError("the episode did not end")


def words(e, ep_rew):
    """the 12 state words the device keeps for this twin"""
    return [e.x, e.xd, e.th, e.thd, e.draws, e.steps, e.ep_steps, ep_rew, e.prev, 0, 0, 0]


@functools.lru_cache(maxsize=None)
def host_play(B, n, rules="plain", cap=60, shift=0, env_id0=7, seed=SEED):
    """B host twins (env ids env_id0 ..) played for n agent steps, restarted after a done as the Runner does.  Envs with an
    even id take hashed actions, envs with an odd id the controller's.  The twins receive raw + shift, the Runner's host path;
    ``acts`` are the raw actions a device pool with ``action_shift = shift`` plays.  -> acts (n, B) int64; rew, done (n, B);
    obs (n + 1, B, 4): row 0 the reset, row t + 1 what step t left (the reset observation after a done); words (n, B, 12): the
    state words after every step; stats (n, 2): dones so far and the rewards they closed; the summed event counts.  Computed
    once per case, left unchanged."""
    envs = [CartPoleEnv(seed=seed, env_id=env_id0 + j, max_episode_steps=cap, **RULES[rules]) for j in range(B)]
    acts = np.zeros((n, B), dtype=np.int64)
    rew, done = np.zeros((n, B), dtype=np.float32), np.zeros((n, B), dtype=np.float32)
    obs, wds = np.zeros((n + 1, B, 4), dtype=np.float32), np.zeros((n, B, 12), dtype=np.int64)
    stats, ep_rew = np.zeros((n, 2), dtype=np.int64), [0] * B
    for j, e in enumerate(envs):
        obs[0, j] = e.reset()[0]
    closed = [0, 0]
    for t in range(n):
        for j, e in enumerate(envs):
            want = controller(e) if e.env_id % 2 else hash32(seed + 1000, e.env_id, t) >> 7 & 1
            if t % 5 == 0:
                want += 2 * (t % 3)                 # the device takes its actions mod 2
            acts[t, j] = want - shift
            o, r, d, _ = e.step(int(acts[t, j]) + shift)
            ep_rew[j] += int(r)
            if d:
                closed[0] += 1
                closed[1] += ep_rew[j]
                ep_rew[j] = 0
                o = e.reset()
            rew[t, j], done[t, j], obs[t + 1, j], wds[t, j] = r, float(d), o[0], words(e, ep_rew[j])
        stats[t] = closed
    events = {k: sum(e.events[k] for e in envs) for k in envs[0].events}
    out = dict(acts=acts, rew=rew, done=done, obs=obs, words=wds, stats=stats, events=events)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---------------------------------------------------------------- 1. determinism and draws
def test_surface_determinism_and_reset_draws():
    env = CartPoleEnv(seed=3, env_id=1)
    assert env.action_space.n == 2 and CartPoleEnv.N_ACTIONS == 2
    with pytest.raises(RuntimeError):
        env.step(0)                               # a new env is reset by its caller, like a gym env
    o = env.reset()
    assert o.shape == (1, 4) and o.dtype == np.float32 and env.draws == 4
    L = cartpole.RESET_L
    assert L == math.floor(0.05 * 2 ** 20)
    assert [env.x, env.xd, env.th, env.thd] == [hash32(3, 1, i) % (2 * L + 1) - L for i in range(4)]
    assert np.array_equal(o[0].astype(np.float64) * 2 ** 20, [env.x, env.xd, env.th, env.thd])
    o2, rew, done, info = env.step(1)
    assert o2.shape == (1, 4) and rew == 1.0 and isinstance(rew, float) and done is False
    # two twins with the same (seed, env_id): identical trajectories; another env_id: another reset
    a, b, c = (CartPoleEnv(seed=9, env_id=i) for i in (4, 4, 5))
    ra, rb, rc = a.reset(), b.reset(), c.reset()
    assert np.array_equal(ra, rb) and not np.array_equal(ra, rc)
    for t in range(300):
        act = hash32(1, 2, t) & 1
        sa, sb = a.step(act), b.step(act)
        assert np.array_equal(sa[0], sb[0]) and sa[1:3] == sb[1:3] and words(a, 0) == words(b, 0)
        if sa[2]:
            assert np.array_equal(a.reset(), b.reset())
    assert a.events == b.events and a.events["episode_end"] >= 5
    # all four reset values of many worlds lie within +-L, and reach both halves of the range
    vals = np.array([[getattr(e, k) for k in ("x", "xd", "th", "thd")] for e in (CartPoleEnv(seed=2, env_id=i) for i in range(500))
                     if e.reset() is not None])
    assert vals.shape == (500, 4) and np.abs(vals).max() <= L and (vals.min(0) < -L // 2).all() and (vals.max(0) > L // 2).all()
    assert len({tuple(v) for v in vals}) == 500


def test_the_constants_are_the_documented_ones():
    cp = cartpole
    assert (cp.FRAC, cp.ONE, cp.CARTPOLE_WORDS, cp.OBS, cp.N_ACTIONS) == (20, 1 << 20, 12, 4, 2)
    real = dict(G=9.8, FORCE=10, PML=0.05, INV_TOTAL=1 / 1.1, MP_TOTAL=0.1 / 1.1, PML_TOTAL=0.05 / 1.1, FOUR_THIRDS=4 / 3, TAU=0.02,
                HALF=0.5, C6=1 / 6, C24=1 / 24, C120=1 / 120, VMAX=8)
    for name, v in real.items():
        assert abs(getattr(cp, name) - v * cp.ONE) <= 0.5, name
    assert cp.X_LIMIT == math.floor(2.4 * cp.ONE) and cp.TH_LIMIT == math.floor(12 * 2 * math.pi / 360 * cp.ONE)
    assert cp.RULE_KEYS == ("frame_skip_max",) and cp.DeviceCartPolePool.frame_shape == (1, 4)
    assert cp.DeviceCartPolePool.needs_actions is True and not hasattr(cp.DeviceCartPolePool, "float_actions")
    # the kernel's header states the same integers
    src = open(os.path.join(ROOT, "pytorch-a2c_amd", "csrc", "cartpole_game.h")).read()
    for name in ("G", "PML", "INV_TOTAL", "MP_TOTAL", "PML_TOTAL", "FOUR_THIRDS", "TAU", "C6", "C24", "C120", "X_LIMIT", "TH_LIMIT",
                 "RESET_L"):
        m = re.search(r"\bCP_%s = (\d+)\b" % name, src)
        assert m and int(m.group(1)) == getattr(cp, name), name


def test_floor_div_is_the_floor():
    for n in (-7, -6, -5, -1, 0, 1, 5, 6, 7, -(1 << 45) - 3, (1 << 45) + 3):
        for d in (1, 2, 3, 6, 651431):
            assert cartpole.floor_div(n, d) == n // d, (n, d)


def test_the_factory_pickles_and_sits_behind_a_sequential_environment():
    from a2c_amd import preprocessing
    from a2c_amd.runner import SequentialEnvironment
    f = pickle.loads(pickle.dumps(CartPoleFactory(env_id=4, seed=2, max_episode_steps=9)))
    env = SequentialEnvironment("CartPole-host", preprocessing.null_prep, seed=2, env_fn=f)
    assert env.is_discrete is True and env.n == 2 and env.raw_shape == (1, 4)
    assert isinstance(env.env, CartPoleEnv) and env.env.env_id == 4 and env.env.max_episode_steps == 9


# ---------------------------------------------------------------- 2. every rule fires
def test_every_cause_ends_an_episode():
    for a in (0, 1):        # a constant push: the pole falls
        e = CartPoleEnv(seed=SEED, env_id=3)
        assert play(e, lambda env, n: a) < 100 and e.events == dict(x_limit=0, theta_limit=1, step_limit=0, episode_end=1)
    e = CartPoleEnv(seed=SEED, env_id=3, max_episode_steps=30)
    assert play(e, lambda env, n: n & 1) == 30 and e.events == dict(x_limit=0, theta_limit=0, step_limit=1, episode_end=1)
    for env_id in (0, 7, 8, 139):       # the controller keeps the pole up; the cart drifts out of the track
        e = CartPoleEnv(seed=SEED, env_id=env_id)
        n = play(e, lambda env, n: controller(env))
        print(f"cartpole controller env {env_id}: x_limit after {n} frames")
        assert e.events["x_limit"] >= 1 and e.events == dict(x_limit=1, theta_limit=0, step_limit=0, episode_end=1) and n < 200


@pytest.mark.parametrize("B", [64, 65, 130])
def test_the_streams_of_the_device_comparison_show_every_cause(B):
    """what test_gpu_cartpole.py plays.  A cart cannot leave the track inside 60 frames without the pole falling first (the
    lean the 12 degree limit allows gives it about 2 m/s^2), so the worlds of max_episode_steps = 60 show theta_limit and
    step_limit, and the same streams on the worlds of 500 add x_limit: every cause is compared on the device"""
    short, full = host_play(B, 600, "plain", 60)["events"], host_play(B, 600, "plain", 500)["events"]
    print(f"cartpole streams B={B}: cap 60 {short}; cap 500 {full}")
    assert short["theta_limit"] >= 1 and short["step_limit"] >= 1 and short["x_limit"] == 0
    assert full["x_limit"] >= 1 and full["theta_limit"] >= 1
    assert all(short[k] + full[k] >= 1 for k in ("x_limit", "theta_limit", "step_limit"))
    rep = {cap: host_play(65, 600, "repeat", cap, 3)["events"] for cap in (60, 500)}
    assert all(rep[60][k] + rep[500][k] >= 1 for k in ("x_limit", "theta_limit", "step_limit", "cut", "sticky")), rep


# ---------------------------------------------------------------- 3. one frame against float64
def _r(k, real):
    """the rounding of a constant, in units"""
    return abs(k - real * cartpole.ONE)


def _mul_err(A, ea, B, eb):
    """units of error of mul(a, b) where |a| <= A carries ea units, |b| <= B carries eb: first order, the cross term, the floor"""
    return A * eb + B * ea + ea * eb * U + 1


def one_step_bound(V=4.0):
    """DESIGN.md section 6k, "the error of one frame": |twin - exact| in units for (x, x_dot, theta, theta_dot) after one frame
    from an exactly representable state with |theta| <= 12 degrees and |x_dot|, |theta_dot| <= V, by the floors on each path
    and the roundings of the constants, each times the magnitudes that multiply it"""
    cp = cartpole
    TH = cp.TH_LIMIT * U
    T2 = TH * TH
    e_t2 = 1.0
    e_ins = _mul_err(T2, e_t2, 1 / 120, _r(cp.C120, 1 / 120)) + _r(cp.C6, 1 / 6)
    e_s = _mul_err(TH, 0, T2 / 6, _mul_err(T2, e_t2, 1 / 6, e_ins)) + TH ** 7 / 5040 / U           # + the series' remainder
    e_inc = _mul_err(T2, e_t2, 1 / 24, _r(cp.C24, 1 / 24))
    e_c = _mul_err(T2, e_t2, 0.5, e_inc) + TH ** 6 / 720 / U
    P1 = V * V * TH
    e_p1 = _mul_err(V * V, 1.0, TH, e_s)
    e_p2 = _mul_err(0.05, _r(cp.PML, 0.05), P1, e_p1)
    SUMF = 10 + 0.05 * P1
    e_temp, TEMP = _mul_err(SUMF, e_p2, 1 / 1.1, _r(cp.INV_TOTAL, 1 / 1.1)), SUMF / 1.1
    e_num = _mul_err(9.8, _r(cp.G, 9.8), TH, e_s) + _mul_err(1.0, e_c, TEMP, e_temp)
    NUM = 9.8 * TH + TEMP
    e_cc = _mul_err(1.0, e_c, 1.0, e_c)
    e_den = (_mul_err(0.1 / 1.1, _r(cp.MP_TOTAL, 0.1 / 1.1), 1.0, e_cc) + _r(cp.FOUR_THIRDS, 4 / 3)) / 2 + 1
    DEN = 0.5 * (4 / 3 - 0.1 / 1.1)                 # the divisor's minimum (cos = 1); DEN - e_den U bounds the computed one
    e_thacc, THACC = e_num / (DEN - e_den * U) + NUM * e_den / (DEN * (DEN - e_den * U)) + 1, NUM / DEN
    e_pt = _mul_err(0.05 / 1.1, _r(cp.PML_TOTAL, 0.05 / 1.1), THACC, _mul_err(THACC, e_thacc, 1.0, e_c))
    e_xacc, XACC = e_temp + e_pt, TEMP + 0.05 / 1.1 * THACC
    rt, tau = _r(cp.TAU, 0.02), cp.TAU * U
    return V * rt + 1, _mul_err(tau, rt, XACC, e_xacc), V * rt + 1, _mul_err(tau, rt, THACC, e_thacc)


def euler64(x, xd, th, thd, a):
    """one explicit Euler step of the equations in float64"""
    f = 10.0 if a else -10.0
    s, c = math.sin(th), math.cos(th)
    temp = (f + 0.05 * thd * thd * s) / 1.1
    thacc = (9.8 * s - c * temp) / (0.5 * (4 / 3 - 0.1 * c * c / 1.1))
    xacc = temp - 0.05 * thacc * c / 1.1
    return x + 0.02 * xd, xd + 0.02 * xacc, th + 0.02 * thd, thd + 0.02 * thacc


def test_one_frame_agrees_with_float64_within_the_derived_bound():
    """12 000 hashed states of the live region (|x| <= 2.4, |theta| <= 12 degrees, |x_dot|, |theta_dot| <= 4), both actions.
    Bound (section 6k): 2.92, 6.24, 2.92, 11.97 units; measured there: 2.88, 5.90, 2.90, 9.87.  The float64 step's own rounding
    is below 1e-8 units"""
    cp = cartpole
    bound = one_step_bound()
    assert [round(b, 2) for b in bound] == [2.92, 6.24, 2.92, 11.97], bound        # the figures section 6k states
    worst, vl = [0.0] * 4, 4 * cp.ONE
    env = CartPoleEnv(seed=0, env_id=0, max_episode_steps=1 << 24)
    for i in range(12000):
        h = [hash32(11, i, k) for k in range(4)]
        st = (h[0] % (2 * cp.X_LIMIT + 1) - cp.X_LIMIT, h[1] % (2 * vl + 1) - vl, h[2] % (2 * cp.TH_LIMIT + 1) - cp.TH_LIMIT,
              h[3] % (2 * vl + 1) - vl)
        for a in (0, 1):
            env.over, env.ep_steps = False, 0
            env.x, env.xd, env.th, env.thd = st
            env._frame(a)
            want = euler64(*(v * U for v in st), a)
            for k, got in enumerate((env.x, env.xd, env.th, env.thd)):
                worst[k] = max(worst[k], abs(got - want[k] / U))
    print(f"cartpole one frame against float64: worst {[round(w, 3) for w in worst]} units, bound {[round(b, 3) for b in bound]}")
    assert all(w <= b + 1e-6 for w, b in zip(worst, bound)), (worst, bound)


def test_the_clamp_and_the_limits():
    cp = cartpole
    x, xd, th, thd = cp.physics(0, cp.VMAX, 0, -cp.VMAX, 1)
    assert xd == cp.VMAX and thd < 0 and abs(thd) <= cp.VMAX
    assert cp.physics(0, 0, cp.TH_LIMIT, cp.VMAX, 0)[3] == cp.VMAX and cp.physics(0, 0, -cp.TH_LIMIT, -cp.VMAX, 1)[3] == -cp.VMAX
    for field, lim in (("x", cp.X_LIMIT), ("th", cp.TH_LIMIT)):
        for v, over in ((lim, False), (lim + 1, True), (-lim, False), (-lim - 1, True)):
            e = CartPoleEnv()
            e.over = False
            setattr(e, field, v)                  # at rest but for the push: one frame moves neither x nor theta
            assert e._frame(0)[1] is over, (field, v)


# ---------------------------------------------------------------- 4. the agent step
@pytest.mark.parametrize("rules", [dict(frame_skip=3), dict(sticky_num=1, sticky_den=4), dict(frame_skip=2, frame_skip_max=4),
                                   dict(frame_skip=3, frame_skip_max=4, sticky_num=1, sticky_den=4)])
def test_agent_step_equals_the_plain_world_frame_by_frame(rules):
    """a plain twin (one frame a step) handed the same draws: the k-draw first, then per game frame the sticky draw before the
    frame; the rewards add up and an over cuts the remaining frames"""
    k0, k1 = rules.get("frame_skip", 1), rules.get("frame_skip_max") or rules.get("frame_skip", 1)
    sn, sd = rules.get("sticky_num", 0), rules.get("sticky_den", 1)
    env, ref = CartPoleEnv(seed=8, env_id=2, max_episode_steps=25, **rules), CartPoleEnv(seed=8, env_id=2, max_episode_steps=25)
    assert np.array_equal(env.reset(), ref.reset())
    prev, cuts = 0, 0
    for t in range(400):
        a = hash32(4, 4, t) % 5                    # taken mod 2
        o, rew, done, _ = env.step(a)
        k = k0 + (ref._draw() % (k1 - k0 + 1) if k1 > k0 else 0)
        assert env.last_k == k
        total, over = 0.0, False
        for s in range(k):
            x = a % 2
            if sn > 0:
                if ref._draw() % sd < sn:
                    x = prev
                prev = x
            ro, r, over, _ = ref.step(x)
            total += r
            if over:
                prev, cuts = 0, cuts + (s < k - 1)
                break
        assert (rew, done) == (total, over) and words(env, 0)[:7] == words(ref, 0)[:7] and np.array_equal(o, ro), t
        assert env.prev == prev and rew == s + 1
        if done:
            assert np.array_equal(env.reset(), ref.reset())
    assert env.events["episode_end"] == ref.events["episode_end"] >= 10
    if k1 > 1:
        assert cuts >= 1 and env.events["cut"] == cuts


# ---------------------------------------------------------------- 5. refusals
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """every argument class of the issue returns A2C_ERR_ARG from the entry points it is an argument of; nothing is launched
    (the addresses are never read: there is no device here)"""
    from a2c_amd import _lib
    lib = _lib.load()
    R, E, HW, C, B = _lib.WorldRules, -1, 4, 2, 2
    A = 1 << 20                                    # a 16-byte aligned address; +4: a misaligned one

    def step(**o):
        a = dict(state=A, actions=A, stride=1, B=B, env0=0, obs=A, obs_ld=HW, rew=A, done=A, reset=A, post=False, val=A,
                 val_prev=A, rewards=A, dones=A, deltas=A, T=3, t=1, C=C, prev=A, prev_stride=C * HW, out=2 * A,
                 out_stride=C * HW, h=None, hdim=0, steps=40, rules=None)
        a.update(o)
        post = _lib.WorldPost(val=a["val"], val_stride=1, val_prev=a["val_prev"], rewards=a["rewards"], dones=a["dones"],
                              deltas=a["deltas"], T=a["T"], t=a["t"], slot0=0, gamma=0.99, pong=0, prev=a["prev"],
                              prev_stride=a["prev_stride"], out=a["out"], out_stride=a["out_stride"], C=a["C"],
                              done_eff_out=None, h=a["h"], hdim=a["hdim"])
        return lib.a2c_cartpole_step(a["state"], a["actions"], a["stride"], 0, a["B"], a["env0"], 1, a["steps"], a["obs"],
                                     a["obs_ld"], a["rew"], a["done"], a["reset"], None, None,
                                     None if a["rules"] is None else ctypes.byref(a["rules"]),
                                     ctypes.byref(post) if a["post"] else None, None)

    def reset(state=A, B=B, env0=0, obs=A, obs_ld=HW, steps=40):
        return lib.a2c_cartpole_reset(state, B, env0, 1, steps, obs, obs_ld, None)
    assert lib.a2c_cartpole_state_bytes() == 48 == 4 * cartpole.CARTPOLE_WORDS
    world = [dict(steps=0), dict(steps=-1), dict(steps=(1 << 24) + 1)]
    common = [dict(B=0), dict(B=-1), dict(env0=-1), dict(state=None), dict(state=A + 4), dict(obs=A + 4), dict(obs_ld=0),
              dict(obs_ld=3), dict(obs_ld=6)]
    for o in world + common + [dict(obs=None)]:
        assert reset(**o) == E, o
    plain = world + common + [dict(obs=None), dict(actions=None), dict(stride=-1), dict(rew=None), dict(done=None),
                              dict(reset=None)]
    plain += [dict(rules=r) for r in (R(0, 0, 0, 1, 0, 0), R(9, 9, 0, 1, 0, 0), R(3, 2, 0, 1, 0, 0), R(2, 9, 0, 1, 0, 0),
                                      R(1, 1, 2, 1, 0, 0), R(1, 1, -1, 4, 0, 0), R(1, 1, 0, 0, 0, 0),
                                      R(1, 1, 0, (1 << 16) + 1, 0, 0), R(1, 1, 0, 1, 1, 0), R(1, 1, 0, 1, 0, 1),
                                      R(2, 4, 1, 4, 1, 0), R(1, 1, 0, 1, 2, 0))]
    for o in plain:
        assert step(**o) == E, o
    posts = [dict(T=0), dict(t=-1), dict(t=3), dict(C=0), dict(prev_stride=C * HW + 2), dict(out_stride=C * HW + 2),
             dict(prev_stride=C * HW - 4), dict(out_stride=C * HW - 4), dict(out=2 * A + 4), dict(prev=A + 8), dict(prev=2 * A),
             dict(h=A, hdim=0), dict(h=A, hdim=-2), dict(obs=A + 4), dict(obs_ld=6)]
    posts += [{n: None} for n in ("val", "val_prev", "rewards", "dones", "deltas", "prev", "out")]
    posts += [o for o in plain if o != dict(obs=None)]
    for o in posts:
        assert step(post=True, **o) == E, o


def test_world_bounds_and_hyps():
    cp = cartpole
    assert world_from_hyps({}) == (500,) and world_from_hyps(dict(max_episode_steps=1 << 24)) == (1 << 24,)
    assert world_from_hyps(dict(max_episode_steps=None)) == (500,) and cp.check_world(1) == (1,)
    for bad in (dict(max_episode_steps=0), dict(max_episode_steps=-3), dict(max_episode_steps=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            world_from_hyps(bad)
        with pytest.raises(ValueError):
            cp.check_world(**bad)
        with pytest.raises(ValueError):
            CartPoleEnv(**bad)
        with pytest.raises(ValueError):
            cp.DeviceCartPolePool(2, "cpu", **bad)            # refused before anything is allocated
    for bad in (dict(frame_skip=0), dict(frame_skip=9), dict(frame_skip=3, frame_skip_max=2), dict(frame_skip_max=9),
                dict(sticky_num=2, sticky_den=1), dict(sticky_num=-1), dict(sticky_den=0), dict(sticky_den=(1 << 16) + 1)):
        with pytest.raises(ValueError):
            cp.check_world(**bad)
        with pytest.raises(ValueError):
            CartPoleEnv(**bad)
        with pytest.raises(ValueError):
            cp.DeviceCartPolePool(2, "cpu", **bad)
    with pytest.raises(ValueError):
        cp.DeviceCartPolePool(0, "cpu")
    with pytest.raises(ValueError):
        cp.DeviceCartPolePool(2, "cpu", env_id0=-1)
    with pytest.raises(TypeError):
        CartPoleEnv(episodic_life=True)                       # keys of the Breakout worlds: not keywords here
    with pytest.raises(TypeError):
        cp.DeviceCartPolePool(2, "cpu", clip_rewards=True)
    assert cp.rules_from_hyps(dict(frame_skip=2, frame_skip_max=4)) == dict(frame_skip_max=4)
    assert cp.rules_from_hyps({}) == dict(frame_skip_max=1)
    for bad in (dict(episodic_life=True), dict(clip_rewards=1), dict(frame_skip=4, frame_skip_max=2)):
        with pytest.raises(ValueError):
            cp.rules_from_hyps(bad)


@pytest.mark.parametrize("env_type,kw", [
    ("CartPole-device", dict(model="A3CModel")), ("CartPole-device", dict(is_discrete=False)),
    ("CartPole-device", dict(episodic_life=1)), ("CartPole-device", dict(eval_pool="device", eval_env=object())),
    ("CartPole-host", dict(clip_rewards=True)), ("CartPole-host", dict(frame_skip_max=9)),
    ("CartPole-device", dict(frame_skip=4, frame_skip_max=2)), ("CartPole-host", dict(model="ConvModel")),
    ("CartPole-host", dict(model="GRUFCModel", is_discrete=False)), ("CartPole-host", dict(eval_pool="device"))])
def test_train_refuses_before_the_device(env_type, kw, tmp_path, monkeypatch):
    import torch
    from a2c_amd.training import train

    def no_device(*a, **k):
        raise AssertionError("train() touched the device")
    monkeypatch.setattr(torch.Tensor, "cuda", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    kw = dict(kw)
    eval_env = kw.pop("eval_env", None)
    hyps = dict(dict(exp_name="cartpole", main_path=str(tmp_path), model="FCModel", env_type=env_type, n_envs=2, n_rollouts=2,
                     n_tsteps=2, n_frame_stack=2, max_tsteps=1e9, seed=1, h_size=16), **kw)
    with pytest.raises(ValueError):
        train(None, hyps, verbose=False, max_epochs=1, eval_env=eval_env)
    assert not list(tmp_path.iterdir()), "nothing was written either"


def test_cartpole_v1_stays_gyms():
    from a2c_amd.training import _WORLDS, _world_family
    assert _world_family("CartPole-device") == _world_family("CartPole-host") == "CartPole" and "CartPole" in _WORLDS
    assert _world_family("CartPole-v1") is None and _world_family("CartPole") is None


# ---------------------------------------------------------------- 6. header and bindings
def test_header_bindings_and_generated_ops():
    from a2c_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "a2c_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("a2c_cartpole_state_bytes", "a2c_cartpole_reset", "a2c_cartpole_step"):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, name
        n_args = 0 if m.group(1).strip() == "void" else len(m.group(1).split(","))
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
    assert len(_lib.SIGNATURES["a2c_cartpole_step"][1]) == 18 and len(_lib.SIGNATURES["a2c_cartpole_reset"][1]) == 8
    assert _lib.SIGNATURES["a2c_cartpole_step"][1][15:17] == [_lib.PU, _lib.PW]
    lib = _lib.load()
    assert lib.a2c_cartpole_state_bytes() == 48
    for f in (ops.cartpole_state_bytes, ops.cartpole_reset, ops.cartpole_step):
        assert callable(f)
    inc = open(os.path.join(ROOT, "pytorch-a2c_amd", "csrc", "torch_ops_abi.inc")).read()
    assert "void abi_cartpole_reset(" in inc and 'm.impl("abi_cartpole_reset", &abi_cartpole_reset)' in inc
    assert re.search(r"// SKIPPED .*\ba2c_cartpole_step\b", inc), "the step takes argument blocks: ctypes, like a2c_point_step"
    mk = open(os.path.join(ROOT, "pytorch-a2c_amd", "csrc", "Makefile")).read()
    assert " cartpole.hip " in mk
