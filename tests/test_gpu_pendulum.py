"""-m gpu: the Pendulum worlds in device memory (csrc/pendulum.hip, a2c_amd.pendulum.DevicePendulumPool) against the host twin
``PendulumEnv`` after every step; sub-ranges of a pool; the post form against its launch sequences; the argument checks; the
floored whole-unit episode sums; the Runner with Gaussian nets (ONE float action) on the device pool against host twins, and
its graph path against the eager loop; the ``DeviceStatsRunner`` against the host ``StatsRunner``; ``train()``.  The world is
integers, the rewards are integers times 2^-8 and the observations are exact fractions, so every comparison is
``torch.equal`` / integer equality."""
import ctypes
import functools
import math
import queue

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import base_hyps  # noqa: E402
from test_pendulum import CAP, REPEAT, RULES, host_play  # noqa: E402

DEV = "cuda"
GAMMA = 0.99
N_STEPS = 200


def dev(a):
    """a (read-only) host array as a device tensor"""
    return torch.from_numpy(np.array(a)).to(DEV)


def _pool(B, rules="plain", seed=5, cap=CAP, **kw):
    from a2c_amd.pendulum import DevicePendulumPool
    return DevicePendulumPool(B, DEV, seed=seed, max_episode_steps=cap, **RULES[rules], **kw)


# ---------------------------------------------------------------- device against twins, after every step
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("shift", [0.0, 0.5])
@pytest.mark.parametrize("rules", list(RULES))
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_device_worlds_equal_the_host_twins(B, rules, shift, strided):
    """max_episode_steps = 7: on the plain world every env of the pool closes in the same step, every seventh"""
    n = N_STEPS
    h = host_play(B, n, rules, shift)
    if B >= 63:      # on the host twins alone: the stream shows the rules, the quantiser's edge values among the actions
        ev = h["events"]
        assert ev["end_cap"] >= B and all(ev[k] > 0 for k in (("cut", "sticky") if rules == "repeat" else ())), ev
        assert np.isnan(h["acts"]).any() and np.isinf(h["acts"]).any()
        assert any(s % 256 for s in h["sums"]), "fractional episode sums: the floor shows"
    pool = _pool(B, rules)
    pool.action_shift = shift
    want = {k: dev(h[k]) for k in ("rew", "done", "obs")}
    want["words"], want["stats"] = dev(h["words"].astype(np.int32)), dev(h["stats"].astype(np.int32))
    if strided:      # env-major rows like a rollout buffer's: act_ld = T, step t at a row offset of t floats
        acts, ld, off = dev(np.ascontiguousarray(h["acts"].T)), n, 4
    else:
        acts, ld, off = dev(h["acts"]), 1, 4 * B
    pool.reset_all()
    assert torch.equal(pool.frames, want["obs"][0]), "reset observations"
    bad = torch.zeros(6, dtype=torch.int64, device=DEV)      # mismatches: words, obs, rew, done, reset, counters
    for t in range(n):
        fr, r, d, rs = pool.step(acts.data_ptr() + off * t, ld)
        bad[0] += (pool.state != want["words"][t]).sum()
        bad[1] += (fr != want["obs"][t + 1]).sum()
        bad[2] += (r != want["rew"][t]).sum()
        bad[3] += (d != want["done"][t]).sum()
        bad[4] += (rs != want["done"][t]).sum()               # real dones only: reset == done
        bad[5] += (pool.ep_stats != want["stats"][t]).sum()
    torch.cuda.synchronize()
    assert bad.tolist() == [0] * 6, bad.tolist()
    assert torch.equal(pool.state, want["words"][-1]) and torch.equal(pool.frames, want["obs"][-1])
    assert pool.episode_stats() == tuple(int(v) for v in h["stats"][-1]) and pool.episode_stats() == (0, 0)
    if rules == "plain":
        assert int(h["stats"][-1][0]) == B * (n // CAP) and float(h["done"][CAP - 1].sum()) == B


def test_the_episode_sum_is_whole_units_floored():
    """ep_rew_sum against the twins' sums: the sum over the closed episodes of each total floored to whole reward units
    (-833.6 -> -834), less than one unit per episode below the exact sum"""
    B, n = 65, 70
    h = host_play(B, N_STEPS, "plain", 0.0)
    pool = _pool(B)
    pool.reset_all()
    acts = dev(h["acts"])
    for t in range(n):
        pool.step(acts[t].data_ptr(), 1)
    k = B * (n // CAP)
    sums = h["sums"][:k]                                      # units of 2^-8, in closing order
    got = pool.episode_stats()
    want = sum(math.floor(s / 256) for s in sums)
    print(f"pendulum episode sums: device {got}, exact {sum(sums) / 256:.4f}, floored {want}")
    assert got == (k, want) and want < sum(sums) / 256 < want + k and want != round(sum(sums) / 256)
    assert torch.equal(pool.state[:, 7], dev(h["words"][n - 1, :, 7].astype(np.int32))), "the running sums stay units of 2^-8"


def test_sub_range_stepping_equals_one_call():
    """env0 / B blocks of a 130-env pool, cut inside and at the end of a wavefront, give what one call gives"""
    B, T = 130, 40
    acts = dev(host_play(B, N_STEPS, "repeat", 0.0)["acts"][:T])
    whole, parts = _pool(B, "repeat"), _pool(B, "repeat")
    whole.reset_all()
    parts.reset_all()
    with pytest.raises(ValueError):
        parts.step(acts[0].data_ptr(), 1, env0=100, B=31)
    for t in range(T):
        whole.step(acts[t].data_ptr(), 1)
        for env0, n in ((0, 64), (64, 1), (65, 65)):
            fr, r, d, rs = parts.device_step(t, env0, n, actions=(acts[t].data_ptr() + 4 * env0, 1))
            assert fr.shape == (n, 4) and r.shape == d.shape == rs.shape == (n,)
        for name in ("state", "frames", "rew", "done", "reset_mask", "ep_stats"):
            assert torch.equal(getattr(whole, name), getattr(parts, name)), (t, name)
    assert int(whole.ep_stats[0]) > 0


# ---------------------------------------------------------------- the post form against its launch sequences
T = 3
POST_STEPS, HDIM = 30, 5


class _Side:
    """one pool and one set of rollout buffers, rows addressed as in the Runner's buffers: slot0 + b, T rows per slot"""

    def __init__(self, B, C, rules, recurrent):
        from a2c_amd import ops
        self.pool = _pool(B, rules)
        self.pool.reset_all()
        self.S, self.slot0 = C * 4, 2
        N = (self.slot0 + B) * T
        f32 = dict(dtype=torch.float32, device=DEV)
        self.states = torch.zeros((N, self.S), **f32)
        self.bookmark = torch.zeros((B, self.S), **f32)
        ops.frame_stack_push(self.pool.frames, torch.ones(B, **f32), self.bookmark.data_ptr(), self.S, self.bookmark.data_ptr(),
                             self.S, B, C, 4)
        self.rewards, self.dones, self.deltas = (torch.full((N,), -7.0, **f32) for _ in range(3))
        self.val_prev, self.done_eff = torch.zeros(B, **f32), torch.full((B,), -7.0, **f32)
        self.h = torch.zeros((B, HDIM), **f32) if recurrent else None

    def sp(self, t):
        return self.states.data_ptr() + 4 * (self.slot0 * T + t) * self.S

    def rows(self, t):
        return (self.sp(t + 1), T * self.S) if t + 1 < T else (self.bookmark.data_ptr(), self.S)

    def tensors(self, frames):
        p = self.pool
        out = dict(state=p.state, rew=p.rew, done=p.done, reset=p.reset_mask, ep_stats=p.ep_stats, rewards=self.rewards,
                   dones=self.dones, deltas=self.deltas, val_prev=self.val_prev, states=self.states, bookmark=self.bookmark)
        if frames:
            out["frames"] = p.frames
        if self.h is not None:
            out.update(h=self.h, done_eff=self.done_eff)
        return out


def _compare_post(B, C, rules, recurrent, obs):
    """one launch == the plain step, then a2c_rollout_post (h == NULL) or a2c_rollout_record + a2c_frame_stack_push"""
    from a2c_amd import ops
    a, b = _Side(B, C, rules, recurrent), _Side(B, C, rules, recurrent)      # a: the launch sequence, b: one launch
    acts = dev(host_play(B, N_STEPS, rules, 0.0)["acts"][:POST_STEPS])
    g = torch.Generator().manual_seed(B * 10 + C)
    vals = torch.randn((POST_STEPS, B, 2), generator=g).to(DEV)              # val_stride = 2
    hs = torch.randn((POST_STEPS, B, HDIM), generator=g).to(DEV)
    S, closed = a.S, 0
    obs0 = b.pool.frames.clone()
    for k in range(POST_STEPS):
        t = k % T
        if t == 0:       # state 0 of a slot = the bookmark
            for x in (a, b):
                x.states.view(-1, T, S)[x.slot0:, 0] = x.bookmark
        if recurrent:
            a.h.copy_(hs[k]); b.h.copy_(hs[k])
        ap, v = (acts[k].data_ptr(), 1), vals[k]
        fr, rew, done, reset = a.pool.device_step(t, 0, B, actions=ap)
        nxt, nstride = a.rows(t)
        if recurrent:
            ops.rollout_record(rew, done, v.data_ptr(), 2, a.val_prev, a.rewards, a.dones, a.deltas, a.done_eff, a.h, B, T, t,
                               a.slot0, GAMMA, False)
            ops.frame_stack_push(fr, reset, a.sp(t), T * S, nxt, nstride, B, C, 4)
        else:
            ops.rollout_post(rew, done, v.data_ptr(), 2, a.val_prev, a.rewards, a.dones, a.deltas, T, t, a.slot0, GAMMA, False, fr,
                             reset, a.sp(t), T * S, nxt, nstride, B, C, 4)
        nxt, nstride = b.rows(t)
        post = ops.world_post(v.data_ptr(), 2, b.val_prev, b.rewards, b.dones, b.deltas, T, t, b.slot0, GAMMA, False, b.sp(t),
                              T * S, nxt, nstride, C, done_eff=b.done_eff if recurrent else None, h=b.h)
        b.pool.device_step_post(t, 0, B, ap, post, frames=obs)
        ta, tb = a.tensors(obs), b.tensors(obs)
        for name in ta:
            assert torch.equal(ta[name], tb[name]), (B, C, k, name)
        if recurrent:
            rows = done.bool()
            assert bool((b.h[rows] == 0).all()) and torch.equal(b.h[~rows], hs[k][~rows])
        closed += int(reset.sum())
    print(f"pendulum post B={B} C={C} {rules} recurrent={recurrent}: closed {closed}, episodes {a.pool.ep_stats.tolist()}")
    assert closed >= B and float(a.deltas[a.slot0 * T:].abs().max()) > 0
    frac = a.rewards[a.slot0 * T:] * 256
    assert torch.equal(frac, frac.round()) and bool((a.rewards[a.slot0 * T:] != a.rewards[a.slot0 * T:].round()).any())
    if not obs:          # obs == NULL: the pool's observation rows were left alone
        assert torch.equal(b.pool.frames, obs0)


@pytest.mark.parametrize("recurrent", [False, True])
@pytest.mark.parametrize("rules", list(RULES))
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("B", [7, 65])
def test_post_form_equals_its_launch_sequence(B, C, rules, recurrent):
    _compare_post(B, C, rules, recurrent, obs=False)


@pytest.mark.parametrize("recurrent", [False, True])
def test_post_form_with_observation_rows(recurrent):
    _compare_post(65, 3, "repeat", recurrent, obs=True)


# ---------------------------------------------------------------- argument checks
def test_argument_checks_return_err_arg_without_launching():
    from a2c_amd import _lib
    lib = _lib.load()
    B, C, HW = 2, 2, 4
    pool = _pool(B, cap=40)
    pool.reset_all()
    f32 = dict(dtype=torch.float32, device=DEV)
    bufs = {n: torch.full((256,), -3.0, **f32) for n in ("out", "prev", "obs", "rew", "done", "reset", "val", "val_prev",
                                                         "rewards", "dones", "deltas", "done_eff", "h")}
    bufs["stats"] = torch.full((64,), -3, dtype=torch.int32, device=DEV)
    acts = torch.zeros((B, 1), **f32)
    ptr = {n: x.data_ptr() + 64 for n, x in bufs.items()}      # 16 floats of canary in front of every output
    R = _lib.WorldRules

    def step(**o):
        a = dict(state=pool.state.data_ptr(), actions=acts.data_ptr(), ld=1, B=B, env0=0, obs=ptr["obs"], obs_ld=HW,
                 rew=ptr["rew"], done=ptr["done"], reset=ptr["reset"], post=False, val=ptr["val"], val_prev=ptr["val_prev"],
                 rewards=ptr["rewards"], dones=ptr["dones"], deltas=ptr["deltas"], T=3, t=1, C=C, prev=ptr["prev"],
                 prev_stride=C * HW, out=ptr["out"], out_stride=C * HW, h=None, hdim=0, steps=40, rules=None)
        a.update(o)
        post = _lib.WorldPost(val=a["val"], val_stride=1, val_prev=a["val_prev"], rewards=a["rewards"], dones=a["dones"],
                              deltas=a["deltas"], T=a["T"], t=a["t"], slot0=0, gamma=GAMMA, pong=0, prev=a["prev"],
                              prev_stride=a["prev_stride"], out=a["out"], out_stride=a["out_stride"], C=a["C"],
                              done_eff_out=ptr["done_eff"], h=a["h"], hdim=a["hdim"])
        return lib.a2c_pendulum_step(a["state"], a["actions"], a["ld"], 0.0, a["B"], a["env0"], 1, a["steps"], a["obs"],
                                     a["obs_ld"], a["rew"], a["done"], a["reset"], ptr["stats"], ptr["stats"] + 4,
                                     None if a["rules"] is None else ctypes.byref(a["rules"]),
                                     ctypes.byref(post) if a["post"] else None, None)

    def reset(state=pool.state.data_ptr(), B=B, env0=0, obs=ptr["obs"], obs_ld=HW, steps=40):
        return lib.a2c_pendulum_reset(state, B, env0, 1, steps, obs, obs_ld, None)
    state0 = pool.state.clone()
    E = -1
    world = [dict(steps=0), dict(steps=-1), dict(steps=(1 << 16) + 1)]
    common = [dict(B=0), dict(B=-1), dict(env0=-1), dict(state=None), dict(state=pool.state.data_ptr() + 4),
              dict(obs=ptr["obs"] + 4), dict(obs_ld=0), dict(obs_ld=6)]
    for o in world + common + [dict(obs=None)]:
        assert reset(**o) == E, o
    plain = world + common + [dict(obs=None), dict(actions=None), dict(actions=acts.data_ptr() + 2), dict(ld=0), dict(ld=-2),
                              dict(rew=None), dict(done=None), dict(reset=None)]
    plain += [dict(rules=r) for r in (R(0, 0, 0, 1, 0, 0), R(9, 9, 0, 1, 0, 0), R(3, 2, 0, 1, 0, 0), R(2, 9, 0, 1, 0, 0),
                                      R(1, 1, 2, 1, 0, 0), R(1, 1, -1, 4, 0, 0), R(1, 1, 0, 0, 0, 0),
                                      R(1, 1, 0, (1 << 16) + 1, 0, 0), R(1, 1, 0, 1, 1, 0), R(1, 1, 0, 1, 0, 1),
                                      R(2, 4, 1, 4, 1, 0), R(1, 1, 0, 1, 2, 0))]
    for o in plain:
        assert step(**o) == E, o
    posts = [dict(T=0), dict(t=-1), dict(t=3), dict(C=0), dict(prev_stride=C * HW + 2), dict(out_stride=C * HW + 2),
             dict(prev_stride=C * HW - 4), dict(out_stride=C * HW - 4), dict(out=ptr["out"] + 4), dict(prev=ptr["prev"] + 8),
             dict(prev=ptr["out"]), dict(h=ptr["h"], hdim=0), dict(h=ptr["h"], hdim=-2), dict(obs=ptr["obs"] + 4),
             dict(obs_ld=6)]
    posts += [{n: None} for n in ("val", "val_prev", "rewards", "dones", "deltas", "prev", "out")]
    posts += [o for o in plain if o != dict(obs=None)]
    for o in posts:
        assert step(post=True, **o) == E, o
    assert lib.a2c_pendulum_state_bytes() == 48
    torch.cuda.synchronize()
    assert torch.equal(pool.state, state0)
    for n, x in bufs.items():
        assert bool((x == -3).all()), n               # nothing ran
    # ... and the valid calls are accepted: plain, post with and without obs, a rules block, hidden rows, a wider act_ld
    assert step() == 0 and step(post=True) == 0 and step(post=True, obs=None) == 0 and step(rules=R(2, 4, 1, 4, 0, 0)) == 0
    assert step(post=True, h=ptr["h"], hdim=5, rules=R(1, 1, 0, 1, 0, 0)) == 0 and step(B=1, ld=7) == 0
    torch.cuda.synchronize()
    assert not torch.equal(pool.state, state0)
    assert reset() == 0
    torch.cuda.synchronize()
    assert bool((bufs["out"][:16] == -3).all()) and bool((bufs["out"][16 + 2 * C * HW:] == -3).all())
    assert bool((bufs["obs"][:16] == -3).all()) and bool((bufs["obs"][16 + B * HW:] == -3).all())
    assert bool((bufs["obs"][16:16 + B * HW] != -3).all())
    assert bool((bufs["h"] == -3).all())              # no env closed: no hidden row was cleared
    for n in ("rew", "done", "reset"):
        assert bool((bufs[n][16 + B:] == -3).all()) and bool((bufs[n][:16] == -3).all()), n
    assert bufs["stats"].tolist() == [-3] * 64        # ... and no episode was counted
    from a2c_amd.pendulum import DevicePendulumPool
    with pytest.raises(ValueError):
        DevicePendulumPool(2, DEV, max_episode_steps=(1 << 16) + 1)


# ---------------------------------------------------------------- through the Runner
RUNNER_B, RUNNER_T, RUNNER_ROUNDS = 5, 6, 5
KINDS = ("FCModel", "GRUFCModel")


def _net(kind, C=4, seed=5):
    import a2c_amd
    torch.manual_seed(seed)
    return getattr(a2c_amd.models, kind)([C, 4], 1, h_size=32, bnorm=False, is_discrete=False)


def _datas(N, net, C=4):
    D = dict(states=torch.zeros(N, C, 4, device=DEV), deltas=torch.zeros(N, device=DEV), rewards=torch.zeros(N, device=DEV),
             dones=torch.zeros(N, device=DEV), actions=torch.zeros(N, 1, device=DEV))
    if net.is_recurrent:
        D["h_states"] = torch.zeros(N, net.h_size, device=DEV)
    return D


def _noise(seed, n, T_=RUNNER_T, B=RUNNER_B):
    """N(0, 1) scaled up so that the quantised actions cover the range, clamps included"""
    g = torch.Generator().manual_seed(seed)
    return (3.0 * torch.randn((n, T_, B, 1), generator=g)).to(DEV)


def _hyps(**kw):
    return base_hyps(**dict(dict(env_type="Pendulum-device", n_tsteps=RUNNER_T, n_rollouts=RUNNER_B, n_envs=RUNNER_B,
                                 is_discrete=False, h_size=32), **kw))


class _LoggedPendulum:
    """a host twin that keeps what every step returned"""

    def __init__(self, **kw):
        from a2c_amd.pendulum import PendulumEnv
        self.env, self.log = PendulumEnv(**kw), []

    def reset(self):
        return self.env.reset()

    def step(self, a):
        obs, rew, done, info = self.env.step(a)
        self.log.append((rew, done))
        return obs, rew, done, info


@functools.lru_cache(maxsize=None)
def runner_pair(kind, rules, shift):
    """the same net, seed and noise: RUNNER_ROUNDS rollouts on a DevicePendulumPool and on a HostEnvPool of host twins"""
    from a2c_amd.pendulum import DevicePendulumPool
    from a2c_amd.runner import HostEnvPool, Runner
    B, hyps = RUNNER_B, _hyps(action_shift=shift)
    eps = _noise(3, RUNNER_ROUNDS)
    out, ema, twins = {}, {}, None
    for which in ("device", "host"):
        net = _net(kind)
        D = _datas(B * RUNNER_T, net)
        if which == "device":
            pool = DevicePendulumPool(B, DEV, seed=12, max_episode_steps=CAP, **RULES[rules])
        else:
            twins = [_LoggedPendulum(seed=12, env_id=j, max_episode_steps=CAP, **RULES[rules]) for j in range(B)]
            pool = HostEnvPool(twins, frame_shape=(1, 4))
        rnd, rq = [0], queue.Queue(1)
        rq.put(0.0)
        r = Runner(D, hyps, None, None, rq, env_pool=pool, normal_fn=lambda t, Bn, env0: eps[rnd[0], t, env0:env0 + Bn])
        rows = []
        for rnd[0] in range(RUNNER_ROUNDS):
            r.rollout(net, list(range(B)), hyps)
            r.finish()
            rows.append({k: v.clone() for k, v in D.items()})
        out[which], ema[which] = rows, rq.get()
    return out, ema, twins


@pytest.mark.parametrize("rules,shift", [("plain", 0.0), ("repeat", 0.5)])
@pytest.mark.parametrize("kind", KINDS)
def test_runner_device_pool_equals_host_twins(kind, rules, shift):
    out, ema, twins = runner_pair(kind, rules, shift)
    log = [x for e in twins for x in e.log]
    print(f"pendulum runner {kind} {rules}: host twins dones={sum(1 for r, d in log if d)} rew_q {ema}")
    assert sum(1 for r, d in log if d) >= RUNNER_B and all(r <= 0 for r, d in log) and any(r != round(r) for r, d in log)
    for k in range(RUNNER_ROUNDS):
        d, h = out["device"][k], out["host"][k]
        for name in h:
            assert torch.equal(d[name], h[name]), (k, name)
    assert out["host"][0]["actions"].shape == (RUNNER_B * RUNNER_T, 1) and float(out["host"][0]["actions"].abs().max()) > 2.0
    # rew_q: the device pool folds the k dones of a rollout into the EMA together and counts whole
    # reward units, every episode's sum floored (section 6l); the host Runner takes the exact sums one at a time.  On the
    # twins' log both rules give the figures the two Runners published
    fold = one = 0.0
    acc = [0.0] * RUNNER_B
    for rnd in range(RUNNER_ROUNDS):
        k = total = 0
        for t in range(RUNNER_T):
            for j, e in enumerate(twins):
                r, d = e.log[rnd * RUNNER_T + t]
                acc[j] += r
                if d:
                    k, total = k + 1, total + math.floor(acc[j])
                    one = .99 * one + .01 * acc[j]
                    acc[j] = 0.0
        if k:
            fold = .99 ** k * fold + (1 - .99 ** k) * total / k
    assert ema["device"] == fold and ema["host"] == one and fold != 0.0 and fold != one


def _play(kind, graphs, update):
    """RUNNER_ROUNDS rollouts (eager, captured, replayed x 3 on the graph path), an update after each -> the rows after
    every rollout, the pool's state words and episode counters, the net's parameters, the graphs made, the launches issued
    per rollout"""
    from a2c_amd import ops
    from a2c_amd.pendulum import DevicePendulumPool
    from a2c_amd.runner import Runner
    eps, rnd = _noise(4, RUNNER_ROUNDS), [0]
    hyps = _hyps(rollout_graphs=graphs, action_shift=0.5)
    net = _net(kind)
    D = _datas(RUNNER_B * RUNNER_T, net)
    pool = DevicePendulumPool(RUNNER_B, DEV, seed=12, max_episode_steps=CAP, **REPEAT)
    r = Runner(D, hyps, None, None, None, env_pool=pool, normal_fn=lambda t, Bn, env0: eps[rnd[0], t, env0:env0 + Bn])
    upd = None
    if update:
        from a2c_amd.updater import Updater
        upd = Updater(net, hyps)
    rows, launches = [], []
    for rnd[0] in range(RUNNER_ROUNDS):
        real, counted = ops.lib, _CountedLib(ops.lib())
        ops.lib = lambda: counted
        try:
            r.rollout(net, list(range(RUNNER_B)), hyps)
        finally:
            ops.lib = real
        r.finish()
        launches.append(counted.n)
        rows.append({k: v.clone() for k, v in D.items()})
        if upd is not None:
            upd.update_model(D)
    torch.cuda.synchronize()
    return (rows, (pool.state.clone(), pool.ep_stats.clone()), [p.detach().clone() for p in net.parameters()],
            list(getattr(r, "_dev_graphs", {}).values()), launches)


class _CountedLib:
    """the ctypes library with every call of a launching a2c_* entry point counted"""

    def __init__(self, lib):
        self._lib, self.n = lib, 0

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("a2c_") or name.endswith(("_bytes", "_supported", "_splits", "_version", "_string")):
            return f

        def counted(*a):
            self.n += 1
            return f(*a)
        return counted


@pytest.mark.parametrize("kind", KINDS)
def test_graph_path_equals_the_eager_loop(kind):
    """five rollouts with an update after each: rows and final parameters equal; a replay issues zero a2c_* calls"""
    got, state, params, made, n = _play(kind, True, True)
    want, state_w, params_w, made_w, n_w = _play(kind, False, True)
    print(f"pendulum {kind}: launches per rollout, graph path {n}, eager {n_w}")
    assert len(made) == 1 and isinstance(made[0], torch.cuda.CUDAGraph) and not made_w      # captured; not on the comparator
    assert n[0] > 0 and n[1] > 0 and n[2:] == [0, 0, 0] and min(n_w) > 0, "a replayed rollout is the replay and nothing else"
    assert int(state_w[1][0]) >= RUNNER_B, "episodes end inside the rollouts"
    for k in range(RUNNER_ROUNDS):
        for name in want[k]:
            assert torch.equal(got[k][name], want[k][name]), (kind, k, name)
    assert torch.equal(state[0], state_w[0]) and torch.equal(state[1], state_w[1])
    for p, q in zip(params, params_w):
        assert torch.equal(p, q)
    assert not torch.equal(want[3]["states"], want[4]["states"])
    assert int(state[0][0, 5]) >= RUNNER_ROUNDS * RUNNER_T, "the replays played new steps"
    plain = _play(kind, False, False)
    assert not torch.equal(params_w[0], plain[2][0]), "the updates changed the weights the later rollouts played with"


def test_runner_refuses_the_wrong_net_or_pool():
    import a2c_amd
    from a2c_amd.pendulum import DevicePendulumPool
    from a2c_amd.runner import DeviceStatsRunner, Runner
    cont = _net("FCModel")
    disc = a2c_amd.models.FCModel([4, 4], 2, h_size=32, bnorm=False)
    two = a2c_amd.models.FCModel([4, 4], 2, h_size=32, bnorm=False, is_discrete=False)
    D = _datas(RUNNER_B * RUNNER_T, cont)
    for net, hyps in ((disc, _hyps(is_discrete=True)), (two, _hyps())):
        with pytest.raises(ValueError):
            Runner(D, hyps, None, None, None, env_pool=DevicePendulumPool(RUNNER_B, DEV)).start(net)
    with pytest.raises(ValueError):
        DeviceStatsRunner(_hyps(), DevicePendulumPool(2, DEV)).rollout(disc)


# ---------------------------------------------------------------- evaluation on the device
@pytest.mark.parametrize("rules", list(RULES))
@pytest.mark.parametrize("kind", KINDS)
def test_device_stats_runner_equals_the_host_stats_runner(kind, rules):
    """the same worlds (env ids 10007 ..) and noise: E episodes on the device against StatsRunner's lock-step loop over host
    twins; max_eval_steps = 20 falls inside the third chunk of 8"""
    from a2c_amd.pendulum import DevicePendulumPool, PendulumEnv
    from a2c_amd.runner import DeviceStatsRunner, StatsRunner
    E, K, cap = 6, 8, 20
    world = dict(max_episode_steps=13 if rules == "plain" else 1000)
    hyps = _hyps(n_test_eps=E, eval_chunk=K, max_eval_steps=cap, action_shift=0.5)
    g = torch.Generator().manual_seed(9)
    eps = (3.0 * torch.randn((2 * cap, E, 1), generator=g)).to(DEV)
    fn = lambda t, En, env0: eps[t, env0:env0 + En]
    net = _net(kind)
    dsr = DeviceStatsRunner(hyps, DevicePendulumPool(E, DEV, seed=4, **world, **RULES[rules]), normal_fn=fn, keep_actions=True)
    for call in range(2):      # the second call plays the next E worlds
        twins = [PendulumEnv(seed=4, env_id=10007 + call * E + j, **world, **RULES[rules]) for j in range(E)]
        got = dsr.rollout(net)
        want = StatsRunner(hyps, envs=twins, normal_fn=fn).rollout(net)
        last = dsr.last
        print(f"pendulum eval {kind} {rules} call {call}: {got} ep_len {last['ep_len'].tolist()} steps {last['steps']}")
        assert got == want and got < 0
        frac = last["ep_rew"].double() * 256
        assert torch.equal(frac, frac.round()) and last["actions"].shape == (last["steps"], E, 1)
        if rules == "plain":      # the world's own cap ends every episode, all in the same step of the second chunk
            assert last["ep_len"].tolist() == [13] * E and int(last["active"].sum()) == 0
            assert (last["steps"], last["chunks"]) == (2 * K, 2)
        else:                     # ... and here the evaluator cuts the episodes short, inside the third chunk
            assert int(last["active"].sum()) == E and int(last["ep_len"].max()) == cap
            assert (last["steps"], last["chunks"]) == (cap, 3)


# ---------------------------------------------------------------- train()
@pytest.mark.parametrize("env_type,key,value", [("Pendulum-device", "eval_pool", "host"), ("Pendulum-device", "eval_pool", "device"),
                                                ("Pendulum-host", "env_pool", "serial"),
                                                ("Pendulum-host", "env_pool", "process_f32")])
@pytest.mark.parametrize("model", KINDS)
def test_train_plays_the_pendulum_env_types(env_type, key, value, model, tmp_path):
    import os
    from a2c_amd.training import train
    hyps = dict(exp_name="pendulum", main_path=str(tmp_path), model=model, env_type=env_type, n_envs=8, n_rollouts=8, n_tsteps=5,
                n_frame_stack=3, max_tsteps=1e9, seed=1, max_episode_steps=9, h_size=32, n_test_eps=2, max_eval_steps=20,
                frame_skip=2, frame_skip_max=3, sticky_num=1, sticky_den=4)
    hyps[key] = value
    seen = []
    best = train(None, hyps, verbose=False, max_epochs=2,
                 on_epoch=lambda epoch, upd, D: seen.append((tuple(D["states"].shape), tuple(D["actions"].shape),
                                                             float(D["states"][:, :, 3].abs().max()), float(D["dones"].sum()),
                                                             # (a slot's last reward carries the bootstrap value)
                                                             float(D["rewards"].view(8, 5)[:, :-1].max()),
                                                             float(D["states"][:, -1, :2].abs().max()))))
    assert len(seen) == 2 and seen[0][0] == (40, 3, 4) and seen[0][1] == (40, 1) and seen[0][2] == 0.0
    assert seen[0][3] + seen[1][3] >= 1 and np.isfinite(best) and best < 0 and seen[0][4] < 0 and 0.7 < seen[0][5] <= 1.0 + 1e-5
    log = open(os.path.join(str(tmp_path), "pendulum", "pendulum_0", "log.txt")).read()
    assert "BestRew:" in log and f"env_type:{env_type}" in log


@pytest.mark.parametrize("env_type,kw", [("Pendulum-device", dict(model="A3CModel")), ("Pendulum-host", dict(model="ConvModel")),
                                         ("Pendulum-device", dict(is_discrete=True)),
                                         ("Pendulum-host", dict(model="GRUFCModel", is_discrete=True)),
                                         ("Pendulum-host", dict(env_pool="process")), ("Pendulum-host", dict(env_pool="thread"))])
def test_train_refuses_a_pixel_model_a_discrete_net_and_an_int_pool(env_type, kw, tmp_path):
    from a2c_amd.training import train
    hyps = dict(dict(exp_name="pendulum", main_path=str(tmp_path), model="FCModel", env_type=env_type, n_envs=2, n_rollouts=2,
                     n_tsteps=2, n_frame_stack=2, max_tsteps=1e9, seed=1, h_size=16), **kw)
    with pytest.raises(ValueError):
        train(None, hyps, verbose=False, max_epochs=1)
    assert not list(tmp_path.iterdir()), "nothing was written"
