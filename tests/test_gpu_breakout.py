"""-m gpu: the Breakout worlds in device memory (csrc/breakout.hip, a2c_amd.breakout.DeviceBreakoutPool) against the host
twin ``BreakoutEnv`` -- value for value --, from planted positions, in sub-ranges of a pool, through the Runner against a
HostEnvPool of host twins, as a captured rollout, the ``rew_q`` folding, and through ``train()``.  Everything the worlds
produce is integers and frames of seven grey levels, so those comparisons are exact; rollout rows are compared the way
test_gpu_pong.py compares them: states, actions and dones exactly, rewards and deltas (which hold the nets' values) to 1e-5."""
import functools
import queue

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import base_hyps, hashf  # noqa: E402
from test_breakout import tracking_action  # noqa: E402
from test_gpu_kernels import close  # noqa: E402
from test_gpu_pong import _datas, _uniforms  # noqa: E402

DEV = "cuda"
HW = 80 * 72
WORDS = 24
LEVELS = (0, 66, 72, 162, 180, 198, 200)
WORLDS = {"two_lives": dict(lives=2), "step_limit": dict(max_episode_steps=150)}
# (world, B) -> (seed of the worlds and of the action tape, steps); chosen ON THE CPU so that the host twins alone show
# every event of EVENTS and every action within that many steps
PARITY = {("two_lives", 1): (4, 600), ("two_lives", 7): (4, 600), ("two_lives", 256): (0, 200),
          ("step_limit", 1): (0, 600), ("step_limit", 7): (0, 600), ("step_limit", 256): (0, 200)}
EVENTS = ("side_wall", "brick", "paddle_hit", "life_lost", "episode_end")


def render_batch(words):
    """(B, 24) integer state words (a tensor on any device) -> the (B, 5760) float32 frames they show: bricks, then the
    paddle, then the ball.  host_play checks it against ``BreakoutEnv.prepped()`` for every twin after every step, so what
    the device frames are compared with ARE the twins' frames; only the state words are kept between steps."""
    w = words.long()
    B, dev = w.shape[0], w.device
    level = torch.tensor([200., 198., 180., 162., 72., 66.], device=dev)
    alive = ((w[:, 11:17, None] >> torch.arange(18, device=dev)) & 1).float()            # (B, 6, 18)
    pic = torch.zeros((B, 80, 72), device=dev)
    pic[:, 11:29] = (alive * level[None, :, None]).repeat_interleave(3, dim=1).repeat_interleave(4, dim=2)
    ys, xs = torch.arange(80, device=dev)[None], torch.arange(72, device=dev)[None]
    px, bx, by = (w[:, k, None] for k in (0, 1, 2))
    paddle = ((ys >= 77) & (ys < 79))[:, :, None] & ((xs >= px) & (xs < px + 8))[:, None, :]
    ball = ((ys >= by) & (ys < by + 2))[:, :, None] & ((xs >= bx) & (xs < bx + 2))[:, None, :]
    return torch.where(paddle | ball, pic.new_tensor(200.), pic).reshape(B, HW)


def play_twins(envs, seed, n):
    """the twins under the tracking policy, reset after a real done like the Runner does -> dict of the recorded actions,
    rew, done (n, B), the state words (n + 1, B, 24: row 0 the start, row t + 1 after step t and its reset), the event
    counts since the start; render_batch of every row of words is checked against the twins' prepped() frames"""
    B = len(envs)
    acts = np.zeros((n, B), dtype=np.int64)
    rew, done = (np.zeros((n, B), dtype=np.float32) for _ in range(2))
    words = np.zeros((n + 1, B, WORDS), dtype=np.int32)
    ev0 = {k: sum(e.events[k] for e in envs) for k in envs[0].events}
    seen = np.zeros(256, dtype=bool)

    def keep(t):
        words[t] = [e.state_words() for e in envs]
        want = np.stack([e.prepped().reshape(-1) for e in envs])
        assert np.array_equal(render_batch(torch.from_numpy(words[t])).numpy(), want), t
        seen[want] = True
    keep(0)
    for t in range(n):
        for j, e in enumerate(envs):
            acts[t, j] = tracking_action(e, seed, j, t)
            r, d = e.advance(int(acts[t, j]))
            if d:
                e.new_episode()
            rew[t, j], done[t, j] = r, float(d)
        keep(t + 1)
    events = {k: sum(e.events[k] for e in envs) - ev0[k] for k in ev0}
    for a in (acts, rew, done, words):
        a.setflags(write=False)
    return dict(acts=acts, rew=rew, done=done, words=words, events=events, levels=set(np.nonzero(seen)[0].tolist()))


@functools.lru_cache(maxsize=None)
def host_play(wname, B):
    """B host twins of one world from their reset: computed once per (world, B) and left unchanged"""
    from a2c_amd.breakout import BreakoutEnv
    seed, n = PARITY[(wname, B)]
    envs = [BreakoutEnv(seed=seed, env_id=j, **WORLDS[wname]) for j in range(B)]
    for e in envs:
        e.new_episode()
    return play_twins(envs, seed, n)


def dev(a):
    """a (read-only) host array as a device tensor"""
    return torch.from_numpy(np.array(a)).to(DEV)


def closed_counters(h):
    """episodes finished so far and the rewards they had collected, after every step: every reward of a twin belongs to the
    episode its next done closes, on top of what the starting position had collected already (state word 10)"""
    rew, done = h["rew"].astype(np.int64), h["done"]
    n, B = rew.shape
    out, run, tot = np.zeros((n, 2), dtype=np.int64), h["words"][0][:, 10].astype(np.int64), np.zeros(2, dtype=np.int64)
    for t in range(n):
        run += rew[t]
        d = done[t] != 0
        tot += (int(d.sum()), int(run[d].sum()))
        run[d] = 0
        out[t] = tot
    return out.astype(np.int32)


def compare_steps(pool, h, n):
    """replays the recorded actions on the device worlds: rew, done, reset, the frame rows, the values of the frames and the
    two counters after every step, the state words after the last"""
    d_acts, d_words = dev(h["acts"]), dev(h["words"])
    want = {k: dev(h[k]) for k in ("rew", "done")}
    levels = torch.tensor(LEVELS, dtype=torch.float32, device=DEV)
    bad = torch.zeros(5, dtype=torch.int64, device=DEV)       # mismatches: rew, done, reset, frames; frame values not in LEVELS
    stats = []
    for t in range(n):
        fr, r, d, rs = pool.step(d_acts[t].data_ptr(), 1)
        bad[0] += (r != want["rew"][t]).sum()
        bad[1] += (d != want["done"][t]).sum()
        bad[2] += (rs != want["done"][t]).sum()
        bad[3] += (fr != render_batch(d_words[t + 1])).sum()
        bad[4] += (fr[:, :, None] != levels).all(dim=2).sum()
        stats.append(pool.ep_stats.clone())
    torch.cuda.synchronize()
    assert bad.tolist() == [0, 0, 0, 0, 0], bad.tolist()
    assert np.array_equal(torch.stack(stats).cpu().numpy(), closed_counters(h)), "finished-episode counters after every step"
    assert np.array_equal(pool.state.cpu().numpy(), h["words"][n]), "state words after the last step"


@pytest.mark.parametrize("B", [1, 7, 256])
@pytest.mark.parametrize("wname", list(WORLDS))
def test_device_worlds_equal_the_host_twins(wname, B):
    from a2c_amd.breakout import DeviceBreakoutPool
    seed, n = PARITY[(wname, B)]
    h = host_play(wname, B)
    counts = np.bincount(h["acts"].reshape(-1), minlength=4)
    print(f"breakout parity {wname} B={B} steps={n}: host twin events {h['events']}, actions {counts}, levels {sorted(h['levels'])}")
    assert n <= 600 and all(h["events"][k] >= 1 for k in EVENTS), h["events"]            # on the host twins alone
    assert counts.min() >= 1 and h["levels"] == set(LEVELS)
    pool = DeviceBreakoutPool(B, DEV, seed=seed, **WORLDS[wname])
    pool.reset_all()
    assert torch.equal(pool.frames, render_batch(dev(h["words"][0]))), "reset frames"
    assert np.array_equal(pool.state.cpu().numpy(), h["words"][0]), "reset state"
    compare_steps(pool, h, n)
    closed = closed_counters(h)
    assert pool.episode_stats() == (int(closed[-1, 0]), int(closed[-1, 1])) and pool.episode_stats() == (0, 0)


@functools.lru_cache(maxsize=None)
def planted_play(n=120):
    """three positions natural play this short does not reach, as twins: one brick left with the ball under it (the wall
    is cleared, a real done), twelve cleared columns with the ball rising at vy = -2 (the ceiling), the lower three rows
    gone with the ball under a row-2 brick (the speed-up)"""
    from a2c_amd.breakout import FULL_ROW, BreakoutEnv
    seed = 9
    plants = [dict(rows=[0, 0, 0, 1 << 7, 0, 0], ball=(28, 24), vel=(1, -1), ep_rew=3, ep_steps=40),
              dict(rows=[FULL_ROW & ~0xFFF] * 6, ball=(40, 30), vel=(-1, -2), ep_rew=0, ep_steps=7),
              dict(rows=[FULL_ROW] * 3 + [0] * 3, ball=(21, 22), vel=(1, -1), ep_rew=12, ep_steps=90)]
    envs = []
    for j, p in enumerate(plants):
        e = BreakoutEnv(seed=seed, env_id=j)
        e.new_episode()
        e.rows, e.bricks_left = list(p["rows"]), sum(bin(m).count("1") for m in p["rows"])
        (e.ball_x, e.ball_y), (e.vx, e.vy) = p["ball"], p["vel"]
        e.ep_rew, e.ep_steps, e.steps = p["ep_rew"], p["ep_steps"], p["ep_steps"]
        twin = BreakoutEnv(seed=seed, env_id=j)      # through the state words, the way the device gets the position
        twin.load_state_words(e.state_words())
        envs.append(twin)
    return seed, play_twins(envs, seed, n)


def test_planted_states_ceiling_speed_up_and_cleared_wall():
    from a2c_amd.breakout import DeviceBreakoutPool
    n = 120
    seed, h = planted_play(n)
    print(f"breakout planted: host twin events {h['events']}")
    assert all(h["events"][k] >= 1 for k in ("cleared", "ceiling", "speed_up", "episode_end")), h["events"]
    assert h["done"][:3, 0].any(), "the last brick goes within three steps"
    pool = DeviceBreakoutPool(3, DEV, seed=seed)
    pool.reset_all()
    pool.state.copy_(dev(h["words"][0]))
    compare_steps(pool, h, n)


def test_action_shift_and_strided_actions():
    """the kernel reads actions[e * stride] + action_shift (taken mod 4), like a row of the rollout buffer"""
    from a2c_amd.breakout import DeviceBreakoutPool
    B, T = 7, 80
    h = host_play("two_lives", B)
    pool = DeviceBreakoutPool(B, DEV, seed=PARITY[("two_lives", B)][0], **WORLDS["two_lives"])
    pool.action_shift = 1
    pool.reset_all()
    buf = torch.from_numpy(np.ascontiguousarray(h["acts"][:T].T) - 5).to(DEV)      # env-major rows; action + shift < 0
    d_words = dev(h["words"])
    for t in range(T):
        fr, r, d, rs = pool.step(buf.data_ptr() + 8 * t, T)
        assert np.array_equal(r.cpu().numpy(), h["rew"][t]) and np.array_equal(d.cpu().numpy(), h["done"][t])
        assert torch.equal(fr, render_batch(d_words[t + 1]))
    assert h["rew"][:T].any() and len(set(h["acts"][:T].reshape(-1).tolist())) == 4


def test_sub_range_stepping_equals_one_call():
    """env0 / B blocks of a 256-env pool give what one call over the pool gives"""
    from a2c_amd.breakout import DeviceBreakoutPool
    B, T = 256, 80
    world = dict(lives=1, max_episode_steps=60)
    d_acts = torch.from_numpy((hashf(T * B, 1005) * 4).astype(np.int64).clip(0, 3).reshape(T, B)).to(DEV)
    whole, parts = DeviceBreakoutPool(B, DEV, seed=5, **world), DeviceBreakoutPool(B, DEV, seed=5, **world)
    whole.reset_all()
    parts.reset_all()
    with pytest.raises(ValueError):
        parts.step(d_acts[0].data_ptr(), 1, env0=200, B=57)
    for t in range(T):
        whole.step(d_acts[t].data_ptr(), 1)
        for env0, n in ((0, 64), (64, 1), (65, 191)):
            fr, r, d, rs = parts.device_step(t, env0, n, actions=(d_acts[t].data_ptr() + 8 * env0, 1))
            assert fr.shape == (n, HW) and r.shape == d.shape == rs.shape == (n,)
        for name in ("state", "frames", "rew", "done", "reset_mask", "ep_stats"):
            assert torch.equal(getattr(whole, name), getattr(parts, name)), (t, name)
    assert int(whole.ep_stats[0]) >= B and int(whole.ep_stats[1]) > 0


def test_argument_checks_return_err_arg_without_launching():
    from a2c_amd import _lib
    lib = _lib.load()
    x = torch.zeros(16384, dtype=torch.int32, device=DEV)      # room for a valid B = 2 launch, should a check let one through
    p = x.data_ptr()

    def step(state=p, actions=p, stride=1, B=2, env0=0, frames=p, ld=HW, rew=p, done=p, reset=p, lives=5, max_steps=10000):
        return lib.a2c_breakout_step(state, actions, stride, 0, B, env0, 1, lives, max_steps, frames, ld, rew, done, reset, None,
                                     None, None)

    def reset(state=p, B=2, env0=0, frames=p, ld=HW, lives=5, max_steps=10000):
        return lib.a2c_breakout_reset(state, B, env0, 1, lives, max_steps, frames, ld, None)
    E = -1
    assert step(lives=0) == E and step(lives=6) == E and reset(lives=0) == E and reset(lives=6) == E and step(lives=-1) == E
    assert step(B=0) == E and step(B=-1) == E and reset(B=0) == E and reset(B=-3) == E
    assert step(state=None) == E and reset(state=None) == E
    assert step(actions=None) == E and step(frames=None) == E and step(rew=None) == E and step(done=None) == E
    assert step(reset=None) == E and reset(frames=None) == E and step(stride=-1) == E and step(env0=-1) == E and reset(env0=-1) == E
    assert step(frames=p + 4) == E and step(ld=HW - 1) == E and step(ld=HW - 4) == E and step(ld=HW + 2) == E
    assert reset(frames=p + 8) == E and reset(ld=HW - 4) == E and reset(ld=HW + 1) == E
    assert step(max_steps=0) == E and step(max_steps=(1 << 24) + 1) == E and reset(max_steps=0) == E
    assert reset(max_steps=(1 << 24) + 1) == E
    assert lib.a2c_breakout_state_bytes(5) == 96 and lib.a2c_breakout_state_bytes(1) == 96
    assert lib.a2c_breakout_state_bytes(0) == 0 and lib.a2c_breakout_state_bytes(6) == 0
    torch.cuda.synchronize()
    assert int(x.abs().sum()) == 0                                             # nothing ran
    from a2c_amd.breakout import DeviceBreakoutPool
    with pytest.raises(ValueError):
        DeviceBreakoutPool(2, DEV, lives=6)
    with pytest.raises(ValueError):
        DeviceBreakoutPool(2, DEV, max_episode_steps=0)
    with pytest.raises(RuntimeError):
        DeviceBreakoutPool(2, DEV).step(p, 1)                                  # not started


# ---------------------------------------------------------------- through the Runner
RUNNER_WORLD = dict(lives=1, max_episode_steps=45)              # every world ends an episode within 45 steps
RUNNER_B, RUNNER_T, RUNNER_ROUNDS = 4, 6, 10                     # 60 steps per env


def _net(kind, ss, seed=5):
    import a2c_amd
    torch.manual_seed(seed)
    return getattr(a2c_amd.models, kind)(list(ss), 4, h_size=64 if kind == "FCModel" else 256, bnorm=False)


class _PreppedBreakout:
    """a host twin handing on breakout_prep'ed frames (SequentialEnvironment would spend one reset on probing the shape);
    keeps what every step returned"""

    def __init__(self, **kw):
        from a2c_amd.breakout import BreakoutEnv
        self.env = BreakoutEnv(**kw)
        self.log = []                             # (reward, real done) of every step

    def reset(self):
        from a2c_amd import preprocessing
        return preprocessing.breakout_prep(self.env.reset())

    def step(self, a):
        from a2c_amd import preprocessing
        obs, rew, done, info = self.env.step(a)
        self.log.append((rew, done))
        return preprocessing.breakout_prep(obs), rew, done, info


def folded_ema(twins, T, n_rounds, ema=0.0):
    """rew_q by the folding rule of DESIGN.md section 6b on what the twins returned: the k episodes that end in a rollout
    enter the EMA together with the mean of their rewards (an episode's rewards may come from earlier rollouts)"""
    run = [0.0] * len(twins)
    for rnd in range(n_rounds):
        k, total = 0, 0.0
        for j, e in enumerate(twins):
            for r, d in e.log[rnd * T:(rnd + 1) * T]:
                run[j] += r
                if d:
                    k, total, run[j] = k + 1, total + run[j], 0.0
        if k:
            ema = .99 ** k * ema + (1 - .99 ** k) * total / k
    return ema


@functools.lru_cache(maxsize=None)
def runner_pair(kind):
    """the same net, seed and uniforms: RUNNER_ROUNDS rollouts with a DeviceBreakoutPool and with a HostEnvPool of host twins"""
    from a2c_amd.breakout import DeviceBreakoutPool
    from a2c_amd.runner import HostEnvPool, Runner
    B, T, ss = RUNNER_B, RUNNER_T, (4, 80, 72)
    hyps = base_hyps(env_type="Breakout-device", n_tsteps=T, n_rollouts=B, n_envs=B)
    us = _uniforms(3, RUNNER_ROUNDS, T, B)
    out, ema, twins = {}, {}, None
    for which in ("device", "host"):
        net = _net(kind, ss)
        D = _datas(B * T, ss)
        if which == "device":
            pool = DeviceBreakoutPool(B, DEV, seed=12, **RUNNER_WORLD)
        else:
            twins = [_PreppedBreakout(seed=12, env_id=j, **RUNNER_WORLD) for j in range(B)]
            pool = HostEnvPool(twins, frame_shape=(1, 80, 72))
        rnd = [0]
        rq = queue.Queue(1)
        rq.put(0.0)
        r = Runner(D, hyps, None, None, rq, env_pool=pool,
                   uniform_fn=lambda t, Bn, env0: us[rnd[0], t, env0:env0 + Bn].contiguous())
        rows = []
        for rnd[0] in range(RUNNER_ROUNDS):
            r.rollout(net, list(range(B)), hyps)
            r.finish()
            rows.append({k: v.clone() for k, v in D.items()})
        out[which], ema[which] = rows, rq.get()
    return out, ema, twins


@pytest.mark.parametrize("kind", ["FCModel", "A3CModel"])
def test_runner_device_pool_equals_host_pool(kind):
    out, ema, twins = runner_pair(kind)
    log = [x for e in twins for x in e.log]
    print(f"breakout runner {kind}: host twins bricks={sum(1 for r, d in log if r != 0)} real dones={sum(1 for r, d in log if d)}")
    assert sum(1 for r, d in log if d) >= RUNNER_B and sum(1 for r, d in log if r != 0) >= 1
    # (an untrained net on grey levels up to 200 has logits tens apart: its softmax leaves most of the mass on few actions)
    assert len({int(a) for rows in out["host"] for a in rows["actions"].tolist()}) >= 2
    assert len(set(out["host"][0]["states"].unique().tolist())) >= 5, "grey levels, not a binary frame"
    for k in range(RUNNER_ROUNDS):
        d, h = out["device"][k], out["host"][k]
        assert torch.equal(d["actions"], h["actions"]), k
        assert torch.equal(d["dones"], h["dones"]), k
        assert torch.equal(d["states"], h["states"]), k
        close("rewards", d["rewards"], h["rewards"].cpu().numpy(), 1e-5, 1e-5)
        close("deltas", d["deltas"], h["deltas"].cpu().numpy(), 1e-5, 1e-5)


def test_rew_q_is_the_folded_ema_of_the_twins_episodes():
    out, ema, twins = runner_pair("FCModel")
    want = folded_ema(twins, RUNNER_T, RUNNER_ROUNDS)
    assert want != 0.0 and abs(ema["device"] - want) < 1e-12, (ema, want)
    assert ema["host"] != 0.0          # the host Runner takes the same episodes one at a time


def test_captured_rollout_replays_new_steps():
    """a rollout captured into a hipGraph and replayed twice == two eager rollouts: the draw, step and episode-step counters
    live in device memory and the kernel advances them"""
    from a2c_amd import ops
    from a2c_amd.breakout import DeviceBreakoutPool
    from a2c_amd.runner import Runner
    world = dict(lives=1, max_episode_steps=25)               # every world restarts inside the replays
    B, T, ss = 8, 12, (4, 80, 72)
    hyps = base_hyps(env_type="Breakout-device", n_tsteps=T, n_rollouts=B, n_envs=B)
    us = _uniforms(8, 1, T, B)[0]

    def make():
        net, D = _net("FCModel", ss), _datas(B * T, ss)
        pool = DeviceBreakoutPool(B, DEV, seed=2, **world)
        r = Runner(D, hyps, None, None, None, env_pool=pool, uniform_fn=lambda t, Bn, env0: us[t, env0:env0 + Bn])
        r.rollout(net, list(range(B)), hyps)          # warm-up (both): rollout 0
        torch.cuda.synchronize()
        return net, D, pool, r
    net, D, pool, r = make()
    eager = []
    for _ in range(2):
        r.rollout(net, list(range(B)), hyps)
        torch.cuda.synchronize()
        eager.append({k: v.clone() for k, v in D.items()})
    state_eager = pool.state.clone()
    net, D, pool, r = make()
    g = torch.cuda.CUDAGraph()
    state0 = pool.state.clone()
    with ops.graph_capture(g):
        r.rollout(net, list(range(B)), hyps)
    torch.cuda.synchronize()
    assert torch.equal(pool.state, state0), "capturing plays nothing"
    for k in range(2):
        g.replay()
        torch.cuda.synchronize()
        for name in ("states", "actions", "dones", "rewards", "deltas"):
            assert torch.equal(D[name], eager[k][name]), (k, name)
    assert torch.equal(pool.state, state_eager)
    assert not torch.equal(eager[0]["states"], eager[1]["states"])
    st = pool.state.cpu().numpy()
    assert (st[:, 8] == 3 * T).all() and (st[:, 9] < st[:, 8]).all() and (st[:, 7] >= 2).all()      # steps, episode steps, draws


@pytest.mark.parametrize("env_type,env_pool", [("Breakout-device", None), ("Breakout-host", "serial"), ("Breakout-host", "raw")])
def test_train_plays_the_breakout_env_types(env_type, env_pool, tmp_path):
    """train() builds the pools from env_type and the lives / max_episode_steps keys, without gym; "raw": worker processes
    hand on the RAW 210 x 160 x 3 frames and hyps['device_prep'] = "breakout_prep" crops them on the device"""
    import os
    from a2c_amd.training import train
    hyps = dict(exp_name="breakout", main_path=str(tmp_path), model="FCModel", env_type=env_type, n_envs=8, n_rollouts=8,
                n_tsteps=5, n_frame_stack=3, max_tsteps=1e9, seed=1, lives=2, max_episode_steps=200, h_size=32,
                n_test_eps=2, max_eval_steps=20)
    if env_pool == "raw":
        hyps.update(device_prep="breakout_prep", n_env_workers=2)
    elif env_pool:
        hyps["env_pool"] = env_pool
    seen = []
    best = train(None, hyps, verbose=False, max_epochs=2,
                 on_epoch=lambda epoch, upd, D: seen.append((tuple(D["states"].shape), int(D["actions"].max()),
                                                             set(D["states"].unique().tolist()))))
    assert len(seen) == 2 and seen[0][0] == (40, 3, 80, 72) and 0 <= seen[0][1] < 4
    assert seen[0][2] == {float(v) for v in LEVELS}
    assert np.isfinite(best)
    log = open(os.path.join(str(tmp_path), "breakout", "breakout_0", "log.txt")).read()
    assert "BestRew:" in log and f"env_type:{env_type}" in log
    for bad in (dict(device_prep="pong_prep"), dict(device_prep="breakout_prep", env_pool="serial"),
                dict(device_prep="breakout_prep", env_type="Breakout-device"), dict(lives=6)):
        with pytest.raises(ValueError):
            train(None, dict(dict(hyps, exp_name="bad", env_type="Breakout-host", env_pool="process"), **bad), verbose=False,
                  max_epochs=1)
