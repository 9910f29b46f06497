"""CPU: time-limit truncation on the lane worlds as far as it goes without a device -- the rule of
``truncated`` / ``final_obs`` on the three host twins (``worlds.LaneHostWorld``), the fp32 statement of a2c_trunc_bootstrap, the
argument checks of the five new entry points (refused before anything is launched), and the ``ValueError`` naming
``bootstrap_truncated`` for everything the key does not cover."""
import ctypes
import os

import numpy as np
import pytest

from a2c_amd import _lib, cartpole, pendulum, point

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the CartPole inputs of tests/test_gpu_world_trunc.py too: under a cap of 12 game frames a constant push falls over before
# the cap (a terminal end) and an alternating one reaches it (a truncated end); test_cartpole_inputs_close_both_ways shows it
CARTPOLE_CAP = 12
PUSH = {"constant": lambda k: 1, "alternating": lambda k: k % 2}


def _own_end(env):
    """the game's OWN end condition on the twin's public state, written out again (not read from the twin's bookkeeping)"""
    if isinstance(env, cartpole.CartPoleEnv):
        return abs(env.x) > cartpole.X_LIMIT or abs(env.th) > cartpole.TH_LIMIT
    if isinstance(env, point.PointEnv):
        return env.got >= env.targets_to_win
    return False


def _action(env, k, rng):
    if isinstance(env, cartpole.CartPoleEnv):
        return int(rng.integers(0, 2))
    return rng.uniform(-1.5, 1.5, size=2 if isinstance(env, point.PointEnv) else 1).astype(np.float32)


MAKE = {
    "cartpole": lambda **kw: cartpole.CartPoleEnv(seed=3, env_id=2, **kw),
    "pendulum": lambda **kw: pendulum.PendulumEnv(seed=3, env_id=2, **kw),
    "point": lambda **kw: point.PointEnv(seed=3, env_id=2, targets_to_win=1, **kw),
}


@pytest.mark.parametrize("repeat", [dict(), dict(frame_skip=2), dict(frame_skip=2, sticky_num=1, sticky_den=4)],
                         ids=["plain", "skip2", "skip2_sticky"])
@pytest.mark.parametrize("cap", [3, 4, 5])
@pytest.mark.parametrize("world", list(MAKE))
def test_twin_rule(world, cap, repeat):
    """every step sets both attributes; truncated == the episode ended at a frame where the limit held and the game's own
    condition did not; final_obs is the observation of the world the step left, a copy of its own.  frame_skip = 2 against
    an odd limit: the limit falls on the first game frame of an agent step, whose second is dropped (``cut``); against the
    even one on the second"""
    env = MAKE[world](max_episode_steps=cap, **repeat)
    assert env.truncated is False and env.final_obs is None
    rng = np.random.default_rng(7)
    obs = env.reset()
    ends = truncs = 0
    for k in range(60):
        before = env.steps
        obs, rew, done, info = env.step(_action(env, k, rng))
        assert info == {} and isinstance(env.truncated, bool)
        assert env.final_obs.dtype == np.float32 and env.final_obs.shape == obs.shape
        assert np.array_equal(env.final_obs, obs) and np.array_equal(env.final_obs, env.obs())
        assert env.final_obs is not obs
        if not done:
            assert env.truncated is False
            continue
        ends += 1
        want = env.ep_steps >= cap and not _own_end(env)
        assert env.truncated is want, (k, env.ep_steps)
        truncs += env.truncated
        assert env.steps - before <= env.frame_skip
        kept = env.final_obs.copy()
        env.reset()
        assert np.array_equal(env.final_obs, kept), "final_obs must survive the reset that follows"
    assert ends >= 60 // cap - 1 and truncs >= 1
    if world == "pendulum":
        assert truncs == ends, "only the limit ends a Pendulum episode"
    if repeat and cap % 2:
        assert env.events["cut"] >= 1, "an odd limit under frame_skip = 2 cuts an agent step"


def _cartpole_closes(push, env_id):
    env = cartpole.CartPoleEnv(seed=5, env_id=env_id, max_episode_steps=CARTPOLE_CAP)
    env.reset()
    out = []
    for k in range(40):
        _, _, done, _ = env.step(PUSH[push](k))
        if done:
            out.append(env.truncated)
            env.reset()
    return out


def test_cartpole_inputs_close_both_ways():
    """a condition on the inputs: the twin alone shows a close of each kind"""
    for env_id in range(5):
        const, alt = _cartpole_closes("constant", env_id), _cartpole_closes("alternating", env_id)
        assert const and not any(const), "a constant push falls over before the cap: terminal"
        assert alt and all(alt), "an alternating push reaches the cap: truncated"


def _point_at(cap, targets, dx):
    """a Point world put where a constant push along x reaches its target on frame 3: the speed grows by 8 a frame (positions
    +8, +24, +48) and a target is reached below 64 cells of Manhattan distance, so dx = 100 is first reached at +48"""
    env = point.PointEnv(seed=1, env_id=0, targets_to_win=targets, max_episode_steps=cap)
    env.reset()
    env.px, env.py, env.vx, env.vy, env.tx, env.ty = 1000, 1000, 0, 0, 1000 + dx, 1000
    hist = []
    for _ in range(3):
        _, rew, done, _ = env.step(np.array([1.0, 0.0], dtype=np.float32))
        hist.append((done, env.truncated, env.got))
        if done:
            break
    return env, hist


def test_point_last_target_on_the_frame_of_the_cap_is_terminal():
    env, hist = _point_at(cap=3, targets=1, dx=100)
    assert hist == [(False, False, 0), (False, False, 0), (True, False, 1)], hist
    assert env.ep_steps == 3 and env.events["end_targets"] == 1 and env.events["end_cap"] == 0
    assert env.final_obs[0, 6] == np.float32(1 / 8) and env.px == 1048
    # the same frames against a target out of reach: the cap alone ends the episode
    env, hist = _point_at(cap=3, targets=1, dx=2000)
    assert hist[-1] == (True, True, 0) and env.events["end_cap"] == 1
    # and the target reached with frames to spare: terminal
    env, hist = _point_at(cap=4, targets=1, dx=100)
    assert hist[-1] == (True, False, 1) and env.ep_steps == 3


@pytest.mark.parametrize("cap", [3, 5])
def test_pendulum_final_obs_is_one_euler_frame_after_the_last_state(cap):
    """a second twin with a cap one larger has not ended after the same frames: its state is the one the first ended in"""
    a = pendulum.PendulumEnv(seed=9, env_id=4, max_episode_steps=cap)
    b = pendulum.PendulumEnv(seed=9, env_id=4, max_episode_steps=cap + 1)
    a.reset(), b.reset()
    rng = np.random.default_rng(1)
    for k in range(cap):
        act = rng.uniform(-2.5, 2.5, size=1).astype(np.float32)
        oa, _, da, _ = a.step(act)
        ob, _, db, _ = b.step(act)
        assert da == (k == cap - 1) and not db
        assert a.truncated == da
    assert (a.th, a.thd) == (b.th, b.thd)
    s, c = pendulum.sincos(b.th)
    want = (np.array([c, s, b.thd, 0], dtype=np.float32) * np.float32(pendulum.UNIT))[None]
    assert np.array_equal(a.final_obs, want) and np.array_equal(a.final_obs, ob)
    first = a.reset()
    assert not np.array_equal(first, a.final_obs), "the restart draws a new world"


def test_fp32_statement_of_trunc_bootstrap():
    """t = gamma * truncs; x_out = x + t * vfin where t != 0, else x: every operation rounded to fp32, in this order"""
    from a2c_amd import ops
    rng = np.random.default_rng(3)
    n = 257
    x = rng.standard_normal(n).astype(np.float32) * 3
    x[:4] = [0.0, -0.0, 1.0, -1.0]
    vf = (rng.standard_normal(n) * 5).astype(np.float32)
    vf[4:7] = [0.0, -0.0, 2.5]
    tr = (rng.random(n) < 0.4).astype(np.float32)
    tr[:4] = [0, 0, 1, 1]
    gamma = 0.99
    got = ops.trunc_bootstrap_host(x, tr, vf, gamma)
    want = np.empty(n, dtype=np.float32)
    g = np.float32(gamma)
    for i in range(n):
        t = np.float32(g * tr[i])
        want[i] = np.float32(x[i] + np.float32(t * vf[i])) if t != 0 else x[i]
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert bool((got[tr == 1] != x[tr == 1]).any())
    # truncs all 0: the inputs bit for bit (a -0 stays a -0), whatever vfin holds
    bad = np.full(n, np.nan, dtype=np.float32)
    same = ops.trunc_bootstrap_host(x, np.zeros(n, dtype=np.float32), bad, gamma)
    assert np.array_equal(same.view(np.uint32), x.view(np.uint32))
    # the single rounding steps: a double-precision evaluation differs from the statement somewhere
    wide = (x.astype(np.float64) + gamma * tr.astype(np.float64) * vf.astype(np.float64)).astype(np.float32)
    assert not np.array_equal(wide, got)


# ---------------------------------------------------------------- the entry points, without a device
def _host_block(n):
    buf = (ctypes.c_float * n)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_entry_points_are_bound_and_check_their_arguments():
    lib = _lib.load()
    for w in ("point", "cartpole", "pendulum"):
        plain, tr = _lib.SIGNATURES[f"a2c_{w}_step"][1], _lib.SIGNATURES[f"a2c_{w}_step_trunc"][1]
        assert tr[:-1] == plain[:-1] + [_lib.PT] and tr[-1] is _lib.P
    keep, p = _host_block(64)       # (host addresses: every call below is refused before anything is launched)
    i64 = (ctypes.c_int64 * 8)()
    pi = ctypes.cast(i64, ctypes.c_void_p)

    def cartpole_call(tr):
        return lib.a2c_cartpole_step_trunc(p, pi, 1, 0, 1, 0, 1, 3, p, 4, p, p, p, None, None, None, None, tr, None)

    T = _lib.WorldTrunc
    assert cartpole_call(None) == -1
    assert cartpole_call(ctypes.byref(T(trunc=None, trunc_stride=1, final_obs=p, final_ld=4))) == -1
    assert cartpole_call(ctypes.byref(T(trunc=p, trunc_stride=1, final_obs=None, final_ld=4))) == -1
    assert cartpole_call(ctypes.byref(T(trunc=p, trunc_stride=0, final_obs=p, final_ld=4))) == -1
    assert cartpole_call(ctypes.byref(T(trunc=p, trunc_stride=1, final_obs=p, final_ld=3))) == -1       # below HW
    assert cartpole_call(ctypes.byref(T(trunc=p, trunc_stride=1, final_obs=p, final_ld=6))) == -1       # not a multiple of 4
    assert cartpole_call(ctypes.byref(T(trunc=p, trunc_stride=1, final_obs=p.value + 4, final_ld=4))) == -1      # alignment
    good = T(trunc=p, trunc_stride=1, final_obs=p, final_ld=4)
    # a good block does not excuse what a2c_cartpole_step rejects: max_episode_steps = 0, B = 0
    assert lib.a2c_cartpole_step_trunc(p, pi, 1, 0, 1, 0, 1, 0, p, 4, p, p, p, None, None, None, None, ctypes.byref(good), None) == -1
    assert lib.a2c_cartpole_step_trunc(p, pi, 1, 0, 0, 0, 1, 3, p, 4, p, p, p, None, None, None, None, ctypes.byref(good), None) == -1
    # Point's observation is 8 floats: final_ld = 4 is below HW there
    assert lib.a2c_point_step_trunc(p, p, 2, 0.0, 1, 0, 1, 1, 3, p, 8, p, p, p, None, None, None, None, ctypes.byref(good),
                                    None) == -1
    assert lib.a2c_pendulum_step_trunc(p, p, 1, 0.0, 1, 0, 1, 3, p, 4, p, p, p, None, None, None, None, None, None) == -1
    # a2c_final_states / a2c_trunc_bootstrap
    assert lib.a2c_final_states(p, p, 1, 4, -1, p, None) == -1 and lib.a2c_final_states(None, p, 1, 4, 1, p, None) == -1
    assert lib.a2c_final_states(p, p, 0, 4, 1, p.value + 64, None) == -1 and lib.a2c_final_states(p, p, 1, 6, 1, p.value + 64, None) == -1
    assert lib.a2c_final_states(p, p, 1, 4, 1, p, None) == -1                                 # out == states
    assert lib.a2c_final_states(p, p.value + 4, 1, 4, 1, p.value + 64, None) == -1            # alignment
    assert lib.a2c_final_states(p, p, 1, 4, 0, p.value + 64, None) == 0                       # no rows: a no-op
    assert lib.a2c_trunc_bootstrap(p, p, p, p, 0.99, -1, p, p, None) == -1
    assert lib.a2c_trunc_bootstrap(p, p, None, p, 0.99, 4, p, p, None) == -1
    assert lib.a2c_trunc_bootstrap(p, p, p, p, 0.99, 0, p, p, None) == 0
    del keep


# ---------------------------------------------------------------- the key
def _hyps(tmp_path, **kw):
    return dict(dict(exp_name="t", main_path=str(tmp_path), model="FCModel", env_type="Pendulum-device", n_envs=2, n_rollouts=2,
                     n_tsteps=3, max_tsteps=1e9, seed=1, bootstrap_truncated=True), **kw)


def test_train_refuses_what_the_key_does_not_cover_before_anything_is_written(tmp_path):
    from a2c_amd.training import DEFAULTS, train
    assert DEFAULTS["bootstrap_truncated"] is False
    bad = [dict(model="GRUFCModel"),                                   # the hidden row is zeroed before anyone can read it
           dict(env_type="Pong-device", model="A3CModel"), dict(env_type="Breakout-device", model="A3CModel"),
           dict(env_type="Snake-device", model="A3CModel"),            # the picture worlds
           dict(env_type="Pendulum-host"), dict(env_type="CartPole-host"), dict(env_type="Point-host"),      # host pools
           dict(env_type="CartPole-v0", prep_fxn="null_prep")]         # gym
    for kw in bad:
        with pytest.raises(ValueError, match="bootstrap_truncated"):
            train(None, _hyps(tmp_path, **kw), verbose=False, max_epochs=1)
    with pytest.raises(ValueError, match="bootstrap_truncated"):       # an env_fn's envs
        train(None, _hyps(tmp_path, env_type="Env"), verbose=False, max_epochs=1, env_fn=lambda j: None)
    assert os.listdir(str(tmp_path)) == []


def test_updater_runner_and_pools_refuse_by_the_key():
    import a2c_amd
    from a2c_amd.runner import check_bootstrap_truncated
    from a2c_amd.updater import Updater
    hyps = dict(optim_type="RMSprop", lr=1e-4, is_discrete=False, bootstrap_truncated=True)
    with pytest.raises(ValueError, match="bootstrap_truncated"):
        Updater(a2c_amd.GRUFCModel([1, 4], 1, h_size=16, is_discrete=False), hyps)
    with pytest.raises(ValueError, match="bootstrap_truncated"):
        check_bootstrap_truncated(dict(env_type="Pendulum-device", model="GRUFCModel"))
    with pytest.raises(ValueError, match="bootstrap_truncated"):
        check_bootstrap_truncated(dict(env_type="Pendulum-device", model="FCModel"), pool=object())       # a host pool
    check_bootstrap_truncated(dict(env_type="CartPole-device", model="FCModel"))
    from a2c_amd import worlds
    assert worlds.DeviceLaneWorldPool.reports_trunc is True and worlds.DeviceWorldPool.reports_trunc is False
