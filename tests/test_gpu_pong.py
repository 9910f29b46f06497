"""-m gpu: the Pong worlds in device memory (csrc/pong.hip, a2c_amd.pong.DevicePongPool) against the host twin ``PongEnv``
-- value for value --, in sub-ranges of a pool, through the Runner against a HostEnvPool of host twins, as a captured
rollout, the ``rew_q`` folding, and through ``train()``.  Everything the worlds produce is integers and frames of 0 and 1,
so those comparisons are exact; rollout rows are compared the way test_gpu_models.py compares rollouts with the oracle:
states, actions and dones exactly, rewards and deltas (which hold the nets' values) to 1e-5."""
import functools
import queue

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import base_hyps, hashf  # noqa: E402
from test_gpu_kernels import close  # noqa: E402

DEV = "cuda"
HW = 80 * 80
N_STEPS = 300
# "first_to_21" keeps the default points_to_win: no score reaches 21 in 300 steps, its episodes end by the step limit
WORLDS = {"first_to_2": dict(points_to_win=2), "first_to_21": dict(points_to_win=21, max_episode_steps=120)}
# (world, B) -> seed of the worlds and of the action tape; chosen ON THE CPU so that the host twins alone show every
# event (EVENTS below) within N_STEPS steps
PARITY_SEEDS = {("first_to_2", 1): 0, ("first_to_2", 7): 0, ("first_to_2", 256): 0,
                ("first_to_21", 1): 2, ("first_to_21", 7): 0, ("first_to_21", 256): 0}
EVENTS = ("agent_point", "opp_point", "wall", "hit_agent", "hit_opp", "episode_end")
STATE_WORDS = ("agent_y", "opp_y", "ball_x", "ball_y", "vx", "vy", "score_agent", "score_opp", "draws", "steps", "ep_steps")


def action_tape(seed, B, n):
    """pre-drawn actions (n, B) in {0, 1, 2} from hashf: independent of the worlds' states"""
    return (hashf(n * B, 1000 + seed) * 3).astype(np.int64).clip(0, 2).reshape(n, B)


@functools.lru_cache(maxsize=None)
def host_play(wname, B, n=N_STEPS):
    """B host twins fed the action tape, reset after a real done like the Runner does -> dict of rew, done (the Pong
    override: rew != 0 or real done), reset (the real done) (n, B); the prepped frames one bit per pixel (n + 1, B, 800):
    frame 0 is the reset frame, frame t + 1 what step t returned (the reset frame after a real done); the event counts; the
    twins' final state words (B, 11).  Computed once per (world, B) and left unchanged."""
    from a2c_amd.pong import PongEnv
    seed = PARITY_SEEDS[(wname, B)]
    acts = action_tape(seed, B, n)
    envs = [PongEnv(seed=seed, env_id=j, **WORLDS[wname]) for j in range(B)]
    bits = np.zeros((n + 1, B, HW // 8), dtype=np.uint8)
    rew, done, reset = (np.zeros((n, B), dtype=np.float32) for _ in range(3))
    for j, e in enumerate(envs):
        e.new_episode()
        bits[0, j] = np.packbits(e.prepped())
    for t in range(n):
        for j, e in enumerate(envs):
            r, d = e.advance(int(acts[t, j]))
            if d:
                e.new_episode()
            bits[t + 1, j] = np.packbits(e.prepped())
            rew[t, j], done[t, j], reset[t, j] = r, float(d or r != 0), float(d)
    events = {k: sum(e.events[k] for e in envs) for k in EVENTS}
    state = np.array([[getattr(e, k) for k in STATE_WORDS] for e in envs], dtype=np.int64)
    for a in (acts, bits, rew, done, reset, state):
        a.setflags(write=False)
    return dict(acts=acts, bits=bits, rew=rew, done=done, reset=reset, events=events, state=state)


def dev(a):
    """a (read-only) host array as a device tensor"""
    return torch.from_numpy(np.array(a)).to(DEV)


def frames_of(bits):
    """(B, 800) packed -> (B, 6400) float32 frames on the device"""
    return torch.from_numpy(np.unpackbits(bits, axis=1)).to(DEV).float()


@pytest.mark.parametrize("B", [1, 7, 256])
@pytest.mark.parametrize("wname", list(WORLDS))
def test_device_worlds_equal_the_host_twins(wname, B):
    from a2c_amd.pong import DevicePongPool
    h = host_play(wname, B)
    print(f"pong parity {wname} B={B}: host twin events {h['events']}, actions {np.bincount(h['acts'].reshape(-1), minlength=3)}")
    assert all(h["events"][k] >= 1 for k in EVENTS), h["events"]            # on the host twins alone
    assert np.bincount(h["acts"].reshape(-1), minlength=3).min() >= 1
    assert (h["done"] != h["reset"]).any(), "done and reset are two values"
    pool = DevicePongPool(B, DEV, seed=PARITY_SEEDS[(wname, B)], **WORLDS[wname])
    d_acts = dev(h["acts"])
    want = {k: dev(h[k]) for k in ("rew", "done", "reset")}
    # dones so far and the rewards they closed, after every step
    closed = np.stack([h["done"].sum(1), (h["rew"] * h["done"]).sum(1)], 1).cumsum(0).astype(np.int32)
    pool.reset_all()
    assert torch.equal(pool.frames, frames_of(h["bits"][0])), "reset frames"
    bad = torch.zeros(5, dtype=torch.int64, device=DEV)       # mismatches: rew, done, reset, frames; frame values not in {0, 1}
    stats = []
    for t in range(N_STEPS):
        fr, r, d, rs = pool.step(d_acts[t].data_ptr(), 1)
        bad[0] += (r != want["rew"][t]).sum()
        bad[1] += (d != want["done"][t]).sum()
        bad[2] += (rs != want["reset"][t]).sum()
        bad[3] += (fr != frames_of(h["bits"][t + 1])).sum()
        bad[4] += ((fr != 0) & (fr != 1)).sum()
        stats.append(pool.ep_stats.clone())
    torch.cuda.synchronize()
    assert bad.tolist() == [0, 0, 0, 0, 0], bad.tolist()
    assert np.array_equal(torch.stack(stats).cpu().numpy(), closed), "finished-episode counters after every step"
    assert np.array_equal(pool.state[:, :len(STATE_WORDS)].cpu().numpy().astype(np.int64) & 0xFFFFFFFF,
                          h["state"] & 0xFFFFFFFF), "state words after the last step"
    assert pool.episode_stats() == (int(closed[-1, 0]), int(closed[-1, 1])) and pool.episode_stats() == (0, 0)


def test_action_shift_and_strided_actions():
    """the kernel reads actions[e * stride] + action_shift (taken mod 3), like a row of the rollout buffer"""
    from a2c_amd.pong import DevicePongPool
    B, T = 7, 60
    h = host_play("first_to_2", B)
    pool = DevicePongPool(B, DEV, seed=PARITY_SEEDS[("first_to_2", B)], **WORLDS["first_to_2"])
    pool.action_shift = 1
    pool.reset_all()
    buf = torch.from_numpy(np.ascontiguousarray(h["acts"][:T].T) - 4).to(DEV)      # env-major rows; action + shift < 0
    for t in range(T):
        fr, r, d, rs = pool.step(buf.data_ptr() + 8 * t, T)
        assert np.array_equal(r.cpu().numpy(), h["rew"][t]) and np.array_equal(d.cpu().numpy(), h["done"][t])
        assert torch.equal(fr, frames_of(h["bits"][t + 1]))


def test_sub_range_stepping_equals_one_call():
    """env0 / B blocks of a 256-env pool give what one call over the pool gives"""
    from a2c_amd.pong import DevicePongPool
    B, T = 256, 80
    world = WORLDS["first_to_2"]
    d_acts = torch.from_numpy(action_tape(5, B, T)).to(DEV)
    whole, parts = DevicePongPool(B, DEV, seed=5, **world), DevicePongPool(B, DEV, seed=5, **world)
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
    assert int(whole.ep_stats[0]) > 0


def test_argument_checks_return_err_arg_without_launching():
    from a2c_amd import _lib
    lib = _lib.load()
    x = torch.zeros(16384, dtype=torch.int32, device=DEV)      # room for a valid B = 2 launch, should a check let one through
    p = x.data_ptr()
    ok = dict(points=21, max_steps=10000, num=3, den=4)

    def step(state=p, actions=p, stride=1, B=2, env0=0, frames=p, ld=HW, rew=p, done=p, reset=p, **w):
        w = dict(ok, **w)
        return lib.a2c_pong_step(state, actions, stride, 0, B, env0, 1, w["points"], w["max_steps"], w["num"], w["den"], frames,
                                 ld, rew, done, reset, None, None, None)

    def reset(state=p, B=2, env0=0, frames=p, ld=HW, **w):
        w = dict(ok, **w)
        return lib.a2c_pong_reset(state, B, env0, 1, w["points"], w["max_steps"], w["num"], w["den"], frames, ld, None)
    E = -1
    assert step(points=0) == E and step(points=22) == E and reset(points=0) == E and reset(points=22) == E
    assert step(B=0) == E and step(B=-1) == E and reset(B=0) == E and reset(B=-3) == E
    assert step(state=None) == E and reset(state=None) == E
    assert step(actions=None) == E and step(frames=None) == E and step(rew=None) == E and step(done=None) == E
    assert step(reset=None) == E and reset(frames=None) == E and step(stride=-1) == E and step(env0=-1) == E and reset(env0=-1) == E
    assert step(frames=p + 4) == E and step(ld=HW - 1) == E and step(ld=HW - 4) == E and step(ld=HW + 2) == E
    assert reset(frames=p + 8) == E and reset(ld=HW - 4) == E
    assert step(max_steps=0) == E and step(max_steps=(1 << 24) + 1) == E and step(den=0) == E and step(den=(1 << 16) + 1) == E
    assert step(num=-1) == E and step(num=5) == E and reset(max_steps=0) == E and reset(den=0) == E and reset(num=5) == E
    assert lib.a2c_pong_state_bytes(21) == 64 and lib.a2c_pong_state_bytes(1) == 64
    assert lib.a2c_pong_state_bytes(0) == 0 and lib.a2c_pong_state_bytes(22) == 0
    torch.cuda.synchronize()
    assert int(x.abs().sum()) == 0                                             # nothing ran
    from a2c_amd.pong import DevicePongPool
    with pytest.raises(ValueError):
        DevicePongPool(2, DEV, points_to_win=22)


# ---------------------------------------------------------------- through the Runner
RUNNER_WORLD = dict(points_to_win=1, max_episode_steps=45)      # every world ends an episode within 45 steps
RUNNER_B, RUNNER_T, RUNNER_ROUNDS = 4, 6, 10                     # 60 steps per env


def _datas(N, ss):
    return dict(states=torch.zeros(N, *ss, device=DEV), deltas=torch.zeros(N, device=DEV),
                rewards=torch.zeros(N, device=DEV), dones=torch.zeros(N, device=DEV),
                actions=torch.zeros(N, dtype=torch.int64, device=DEV))


def _net(kind, ss, seed=5):
    import a2c_amd
    torch.manual_seed(seed)
    return getattr(a2c_amd.models, kind)(list(ss), 3, h_size=64 if kind == "FCModel" else 256, bnorm=False)


def _uniforms(seed, n, T, B):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, T, B), generator=g).to(DEV)


class _PreppedPong:
    """a host twin handing on pong_prep'ed frames (SequentialEnvironment would spend one reset on probing the shape);
    keeps what every step returned"""

    def __init__(self, **kw):
        from a2c_amd.pong import PongEnv
        self.env = PongEnv(**kw)
        self.log = []                             # (reward, real done) of every step

    def reset(self):
        from a2c_amd import preprocessing
        return preprocessing.pong_prep(self.env.reset())

    def step(self, a):
        from a2c_amd import preprocessing
        obs, rew, done, info = self.env.step(a)
        self.log.append((rew, done))
        return preprocessing.pong_prep(obs), rew, done, info


def folded_ema(twins, T, n_rounds, ema=0.0):
    """rew_q by the folding rule of DESIGN.md section 6b on what the twins returned: the k dones of a rollout (rew != 0 or
    real done) enter the EMA together with the mean of the rewards they closed"""
    for rnd in range(n_rounds):
        steps = [x for e in twins for x in e.log[rnd * T:(rnd + 1) * T]]
        k = sum(1 for r, d in steps if d or r != 0)
        total = sum(r for r, d in steps)          # a reward closes its own episode: nothing carries over
        if k:
            ema = .99 ** k * ema + (1 - .99 ** k) * total / k
    return ema


@functools.lru_cache(maxsize=None)
def runner_pair(kind):
    """the same net, seed and uniforms: RUNNER_ROUNDS rollouts with a DevicePongPool and with a HostEnvPool of host twins"""
    from a2c_amd.pong import DevicePongPool
    from a2c_amd.runner import HostEnvPool, Runner
    B, T, ss = RUNNER_B, RUNNER_T, (4, 80, 80)
    hyps = base_hyps(env_type="Pong-device", n_tsteps=T, n_rollouts=B, n_envs=B)
    us = _uniforms(3, RUNNER_ROUNDS, T, B)
    out, ema, twins = {}, {}, None
    for which in ("device", "host"):
        net = _net(kind, ss)
        D = _datas(B * T, ss)
        if which == "device":
            pool = DevicePongPool(B, DEV, seed=12, **RUNNER_WORLD)
        else:
            twins = [_PreppedPong(seed=12, env_id=j, **RUNNER_WORLD) for j in range(B)]
            pool = HostEnvPool(twins, frame_shape=(1, 80, 80))
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
    print(f"pong runner {kind}: host twins points={sum(1 for r, d in log if r != 0)} real dones={sum(1 for r, d in log if d)}")
    assert sum(1 for r, d in log if d) >= RUNNER_B and sum(1 for r, d in log if r != 0) >= 1
    assert len({int(a) for rows in out["host"] for a in rows["actions"].tolist()}) == 3
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
    assert ema["host"] != 0.0          # the host Runner takes the same episodes one at a time (runner.py:216)


def test_captured_rollout_replays_new_steps():
    """a rollout captured into a hipGraph and replayed twice == two eager rollouts: the draw, step and episode-step counters
    live in device memory and the kernel advances them"""
    from a2c_amd import ops
    from a2c_amd.pong import DevicePongPool
    from a2c_amd.runner import Runner
    world = dict(points_to_win=1, max_episode_steps=25)      # every world restarts inside the replays
    B, T, ss = 8, 12, (4, 80, 80)
    hyps = base_hyps(env_type="Pong-device", n_tsteps=T, n_rollouts=B, n_envs=B)
    us = _uniforms(8, 1, T, B)[0]

    def make():
        net, D = _net("FCModel", ss), _datas(B * T, ss)
        pool = DevicePongPool(B, DEV, seed=2, **world)
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
    assert (st[:, 9] == 3 * T).all() and (st[:, 10] < st[:, 9]).all() and (st[:, 8] > 3 * T).all()      # steps, episode steps, draws


@pytest.mark.parametrize("env_type,env_pool", [("Pong-device", None), ("Pong-host", "serial")])
def test_train_plays_the_pong_env_types(env_type, env_pool, tmp_path):
    """train() builds the pools from env_type and the points_to_win / max_episode_steps / opp_skill_* keys, without gym"""
    import os
    from a2c_amd.training import train
    hyps = dict(exp_name="pong", main_path=str(tmp_path), model="FCModel", env_type=env_type, n_envs=8, n_rollouts=8,
                n_tsteps=5, n_frame_stack=3, max_tsteps=1e9, seed=1, points_to_win=2, max_episode_steps=200, h_size=32,
                n_test_eps=2, max_eval_steps=20)
    if env_pool:
        hyps["env_pool"] = env_pool
    seen = []
    best = train(None, hyps, verbose=False, max_epochs=2,
                 on_epoch=lambda epoch, upd, D: seen.append((tuple(D["states"].shape), int(D["actions"].max()),
                                                             set(D["states"].unique().tolist()))))
    assert len(seen) == 2 and seen[0][0] == (40, 3, 80, 80) and 0 <= seen[0][1] < 3 and seen[0][2] == {0.0, 1.0}
    assert np.isfinite(best)
    log = open(os.path.join(str(tmp_path), "pong", "pong_0", "log.txt")).read()
    assert "BestRew:" in log and f"env_type:{env_type}" in log
