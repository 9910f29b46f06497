"""-m gpu: the Snake worlds in device memory (csrc/snake.hip, a2c_amd.snake.DeviceSnakePool) against the host twin
``SnakeEnv`` -- value for value --, through the Runner against a HostEnvPool of host twins, as a captured rollout, and a
learning sanity check.  Rollout rows are compared the way test_gpu_models.py compares rollouts with the oracle: states,
actions and dones exactly, rewards and deltas to 1e-5."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import base_hyps  # noqa: E402
from test_gpu_kernels import close  # noqa: E402

DEV = "cuda"
WORLDS = {"default": dict(grid_size=15, unit_size=4, n_foods=2), "21x21": dict(grid_size=21, unit_size=4, n_foods=3)}
N_STEPS = 300
# (world, B) -> seed of the world and of the action tape; chosen ON THE CPU (host_counts below) so that the host twins
# show at least 5 deaths and at least 5 foods in N_STEPS steps
PARITY_SEEDS = {("default", 1): 35, ("default", 7): 0, ("default", 256): 0,
                ("21x21", 1): 0, ("21x21", 7): 0, ("21x21", 256): 0}


def action_tape(seed, B, n):
    """pre-drawn actions (n, B), biased: a step never reverses the one before it (so the neck rarely kills and the
    snakes live long enough to find food), otherwise uniform.  Independent of the worlds' states."""
    from a2c_amd.snake import hash32
    a = np.zeros((n, B), dtype=np.int64)
    for j in range(B):
        prev = hash32(seed, 1000 + j, 0) & 3
        for t in range(n):
            d = hash32(seed, 1000 + j, 1 + t) % 3           # one of the three non-reversing moves
            prev = a[t, j] = (prev + 3 + d) % 4             # prev-1, prev, prev+1
    return a


def host_play(seed, B, world, acts):
    """B host twins fed acts (n, B), resetting after a done like the Runner does -> rew, done (n, B), raw frames
    (n+1, B, H, W, 3): frame 0 is the reset frame, frame t+1 what step t returned (the reset frame after a done)"""
    from a2c_amd.snake import SnakeEnv
    envs = [SnakeEnv(seed=seed, env_id=j, **world) for j in range(B)]
    n = acts.shape[0]
    side = world["grid_size"] * world["unit_size"]
    raw = np.zeros((n + 1, B, side, side, 3), dtype=np.uint8)
    rew, done = np.zeros((n, B), dtype=np.float32), np.zeros((n, B), dtype=np.float32)
    for j, e in enumerate(envs):
        raw[0, j] = e.reset()
    for t in range(n):
        for j, e in enumerate(envs):
            obs, r, d, _ = e.step(int(acts[t, j]))
            if d:
                obs = e.reset()
            raw[t + 1, j], rew[t, j], done[t, j] = obs, r, d
    return rew, done, raw


def host_counts(wname, B):
    """(deaths, foods) of the host twins on the parity tape: what PARITY_SEEDS was chosen by"""
    seed = PARITY_SEEDS[(wname, B)]
    rew, done, _ = host_play(seed, B, WORLDS[wname], action_tape(seed, B, N_STEPS))
    return int((rew < 0).sum()), int((rew > 0).sum())


@pytest.mark.parametrize("B", [1, 7, 256])
@pytest.mark.parametrize("wname", list(WORLDS))
def test_device_worlds_equal_the_host_twins(wname, B):
    from a2c_amd import preprocessing
    from a2c_amd.snake import DeviceSnakePool
    world, seed = WORLDS[wname], PARITY_SEEDS[(wname, B)]
    acts = action_tape(seed, B, N_STEPS)
    rew, done, raw = host_play(seed, B, world, acts)
    deaths, foods = int((rew < 0).sum()), int((rew > 0).sum())
    print(f"snake parity {wname} B={B}: host twin deaths={deaths} foods={foods}")
    assert deaths >= 5 and foods >= 5
    pool = DeviceSnakePool(B, DEV, seed=seed, raw_frames=True, **world)
    d_acts = torch.from_numpy(acts).to(DEV)
    pool.reset()
    torch.cuda.synchronize()
    prep = lambda pics: np.stack([preprocessing.snake_prep(p)[0] for p in pics]).reshape(B, -1)
    assert np.array_equal(pool.rgb.cpu().numpy(), raw[0]), "reset frames"
    assert np.array_equal(pool.frames.cpu().numpy(), prep(raw[0]))
    got = dict(rew=[], done=[], reset=[], rgb=[], frames=[])
    for t in range(N_STEPS):
        fr, r, d, rs = pool.step(d_acts[t].data_ptr(), 1)
        for k, v in (("rew", r), ("done", d), ("reset", rs), ("rgb", pool.rgb), ("frames", fr)):
            got[k].append(v.clone())
    torch.cuda.synchronize()
    g = {k: torch.stack(v).cpu().numpy() for k, v in got.items()}
    assert (g["rew"] < 0).sum() > 0 and (g["rew"] > 0).sum() > 0
    assert np.array_equal(g["rew"], rew) and np.array_equal(g["done"], done) and np.array_equal(g["reset"], done)
    for t in range(N_STEPS):
        assert np.array_equal(g["rgb"][t], raw[t + 1]), f"raw frames of step {t}"
        assert np.array_equal(g["frames"][t], prep(raw[t + 1])), f"prepped frames of step {t}"
    n, s = pool.episode_stats()
    assert n == int(done.sum())


def test_action_shift_and_strided_actions():
    """the kernel reads actions[e * stride] + action_shift, like a row of the rollout buffer"""
    from a2c_amd.snake import DeviceSnakePool
    B, T = 5, 4
    world = WORLDS["default"]
    acts = action_tape(4, B, T)
    rew, done, raw = host_play(9, B, world, acts)
    pool = DeviceSnakePool(B, DEV, seed=9, raw_frames=True, **world)
    pool.action_shift = 1
    pool.reset()
    buf = torch.from_numpy(np.ascontiguousarray(acts.T) - 1).to(DEV)       # (B, T): env-major rows, shifted by -1
    for t in range(T):
        _, r, d, _ = pool.step(buf.data_ptr() + 8 * t, T)
        assert np.array_equal(r.cpu().numpy(), rew[t]) and np.array_equal(d.cpu().numpy(), done[t])
        assert np.array_equal(pool.rgb.cpu().numpy(), raw[t + 1])


def test_argument_checks_return_err_arg_without_launching():
    from a2c_amd import _lib
    lib = _lib.load()
    x = torch.zeros(4096, dtype=torch.int32, device=DEV)
    p = x.data_ptr()
    ok = dict(G=15, unit=4, n_foods=2)

    def step(state=p, actions=p, stride=1, B=2, env0=0, rew=p, done=p, reset=p, frames=p, **w):
        w = dict(ok, **w)
        return lib.a2c_snake_step(state, actions, stride, 0, B, env0, 1, w["G"], w["unit"], w["n_foods"], rew, done, reset,
                                  frames, None, None, None)

    def reset(state=p, B=2, frames=p, **w):
        w = dict(ok, **w)
        return lib.a2c_snake_reset(state, B, 0, 1, w["G"], w["unit"], w["n_foods"], frames, None, None)
    E = -1
    assert step(G=5, unit=1) == E and reset(G=5, unit=1) == E                  # HW = 25: not a multiple of 4
    assert step(n_foods=15 * 15 - 3) == E and reset(n_foods=15 * 15 - 3) == E  # n_foods >= G*G - 3
    assert step(n_foods=0) == E and step(G=3) == E and step(G=33) == E and step(unit=0) == E and step(unit=17) == E
    assert step(state=None) == E and step(actions=None) == E and step(rew=None) == E and step(done=None) == E
    assert step(reset=None) == E and step(frames=None) == E and step(B=-1) == E and step(stride=-1) == E
    assert step(env0=-1) == E and reset(state=None) == E and reset(frames=None) == E and reset(B=-1) == E
    assert step(B=0) == 0 and reset(B=0) == 0
    assert lib.a2c_snake_state_bytes(15, 2) == 4 * (8 + 225) and lib.a2c_snake_state_bytes(15, 222) == 0
    assert lib.a2c_snake_state_bytes(3, 1) == 0 and lib.a2c_snake_state_bytes(33, 1) == 0
    torch.cuda.synchronize()
    assert int(x.abs().sum()) == 0                                             # nothing ran


# ---------------------------------------------------------------- through the Runner
def _datas(N, ss):
    return dict(states=torch.zeros(N, *ss, device=DEV), deltas=torch.zeros(N, device=DEV),
                rewards=torch.zeros(N, device=DEV), dones=torch.zeros(N, device=DEV),
                actions=torch.zeros(N, dtype=torch.int64, device=DEV))


def _net(kind, ss, seed=5):
    import a2c_amd
    torch.manual_seed(seed)
    return getattr(a2c_amd.models, kind)(list(ss), 4, h_size=64 if kind == "FCModel" else 256, bnorm=False)


def _uniforms(seed, n, T, B):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, T, B), generator=g).to(DEV)


class _PreppedSnake:
    """a host twin handing on snake_prep'ed frames (SequentialEnvironment would spend one reset on probing the shape)"""

    def __init__(self, **kw):
        from a2c_amd.snake import SnakeEnv
        self.env = SnakeEnv(**kw)

    def reset(self):
        from a2c_amd import preprocessing
        return preprocessing.snake_prep(self.env.reset())

    def step(self, a):
        from a2c_amd import preprocessing
        obs, rew, done, info = self.env.step(a)
        return preprocessing.snake_prep(obs), rew, done, info


def _host_pool(seed, B, world):
    from a2c_amd.runner import HostEnvPool
    side = world["grid_size"] * world["unit_size"]
    return HostEnvPool([_PreppedSnake(seed=seed, env_id=j, **world) for j in range(B)], frame_shape=(1, side, side))


@pytest.mark.parametrize("kind,wname", [("FCModel", "default"), ("A3CModel", "21x21")])
def test_runner_device_pool_equals_host_pool(kind, wname):
    """the same net, seed and uniforms: a rollout with DeviceSnakePool == one with a HostEnvPool of SnakeEnvs"""
    import queue
    from a2c_amd.runner import Runner
    from a2c_amd.snake import DeviceSnakePool
    world = WORLDS[wname]
    side = world["grid_size"] * world["unit_size"]
    B, T, n_rounds, ss = 6, 9, 3, (4, side, side)
    hyps = base_hyps(env_type="Snake", n_tsteps=T, n_rollouts=B, n_envs=B)
    us = _uniforms(3, n_rounds, T, B)
    N = B * T
    out, ema = {}, {}
    for which in ("device", "host"):
        net = _net(kind, ss)
        D = _datas(N, ss)
        pool = DeviceSnakePool(B, DEV, seed=12, **world) if which == "device" else _host_pool(12, B, world)
        rnd = [0]
        rq = queue.Queue(1)
        rq.put(0.0)
        r = Runner(D, hyps, None, None, rq, env_pool=pool,
                   uniform_fn=lambda t, Bn, env0: us[rnd[0], t, env0:env0 + Bn].contiguous())
        rows = []
        for rnd[0] in range(n_rounds):
            r.rollout(net, list(range(B)), hyps)
            r.finish()
            rows.append({k: v.clone() for k, v in D.items()})
        out[which], ema[which] = rows, rq.get()
    n_done = sum(float(x["dones"].sum()) for x in out["host"])
    assert n_done > 0
    for k in range(n_rounds):
        d, h = out["device"][k], out["host"][k]
        assert torch.equal(d["actions"], h["actions"]), k
        assert torch.equal(d["dones"], h["dones"]), k
        assert torch.equal(d["states"], h["states"]), k
        close("rewards", d["rewards"], h["rewards"].cpu().numpy(), 1e-5, 1e-5)
        close("deltas", d["deltas"], h["deltas"].cpu().numpy(), 1e-5, 1e-5)
    # rew_q: both pools fold the finished episodes into the EMA (the device pool: all episodes of a rollout at once)
    assert ema["device"] != 0.0 and ema["host"] != 0.0


def test_captured_rollout_replays_new_steps():
    """a rollout captured into a hipGraph and replayed twice == two eager rollouts: the draw and step counters live in
    device memory and the kernel advances them"""
    from a2c_amd import ops
    from a2c_amd.runner import Runner
    from a2c_amd.snake import DeviceSnakePool
    world = WORLDS["default"]
    side = world["grid_size"] * world["unit_size"]
    B, T, ss = 16, 12, (4, side, side)
    hyps = base_hyps(env_type="Snake", n_tsteps=T, n_rollouts=B, n_envs=B)
    us = _uniforms(8, 1, T, B)[0]
    N = B * T

    def make():
        net, D = _net("FCModel", ss), _datas(N, ss)
        pool = DeviceSnakePool(B, DEV, seed=2, **world)
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
    assert float(eager[0]["dones"].sum() + eager[1]["dones"].sum()) > 0


# ---------------------------------------------------------------- learning sanity
LEARN_EPOCHS = 1500         # chosen on the MI355X so that the test stays under about a minute (DESIGN.md "Snake")
EVAL_ENVS, EVAL_T, EVAL_ROUNDS = 64, 50, 4          # 64 * 200 = 12 800 evaluation steps per policy


def random_policy_per_env_means(seed, B, n, world):
    """mean reward per step of the uniform-random policy, per env, on the host twins of the evaluation worlds"""
    from a2c_amd.snake import hash32
    acts = np.array([[hash32(seed ^ 0x5EED, j, t) & 3 for j in range(B)] for t in range(n)], dtype=np.int64)
    rew, _, _ = host_play(seed, B, world, acts)
    return rew.mean(0)


def test_learning_beats_the_random_policy():
    """FCModel on Snake-device worlds, RMSprop, the reference's coefficients (hyperparams.json: lr 1e-4, gamma .99,
    lambda .98, val_coef .5, entr_coef .005, max_norm .5, 12-step rollouts, 3 stacked frames): after LEARN_EPOCHS
    epochs the trained policy's mean reward per step on fresh worlds exceeds the uniform-random policy's on the same
    worlds (host twins) by more than three standard errors of the difference (envs are the independent units)."""
    from a2c_amd.runner import Runner
    from a2c_amd.snake import DeviceSnakePool
    from a2c_amd.updater import Updater
    world = WORLDS["default"]
    side = world["grid_size"] * world["unit_size"]
    ss = (3, side, side)
    B, T = 64, 12
    hyps = base_hyps(env_type="Snake-device", n_tsteps=T, n_rollouts=B, n_envs=B, n_frame_stack=3, gamma=.99, lambda_=.98,
                     val_coef=.5, entr_coef=.005, pi_coef=1.0, max_norm=.5, lr=1e-4, optim_type="RMSprop", norm_advs=True)
    import a2c_amd
    torch.manual_seed(0)
    net = a2c_amd.FCModel(list(ss), 4, h_size=256)
    D = _datas(B * T, ss)
    r = Runner(D, hyps, None, None, None, env_pool=DeviceSnakePool(B, DEV, seed=100, **world))
    upd = Updater(net, hyps)
    for _ in range(LEARN_EPOCHS):
        r.rollout(net, list(range(B)), hyps)
        r.finish()
        upd.update_model(D)
    # evaluation: fresh worlds (another seed), the training sampler, no updates
    eval_seed = 4242
    ehyps = dict(hyps, n_tsteps=EVAL_T, n_rollouts=EVAL_ENVS, n_envs=EVAL_ENVS)
    De = _datas(EVAL_ENVS * EVAL_T, ss)
    re_ = Runner(De, ehyps, None, None, None, env_pool=DeviceSnakePool(EVAL_ENVS, DEV, seed=eval_seed, **world))
    tot = torch.zeros(EVAL_ENVS, device=DEV, dtype=torch.float64)
    for _ in range(EVAL_ROUNDS):
        re_.rollout(net, list(range(EVAL_ENVS)), ehyps)
        re_.finish()
        tot += De["rewards"].reshape(EVAL_ENVS, EVAL_T).double().sum(1)
    n = EVAL_T * EVAL_ROUNDS
    assert EVAL_ENVS * n >= 2000
    trained = (tot / n).cpu().numpy()
    rand = random_policy_per_env_means(eval_seed, EVAL_ENVS, n, world)
    se = float(np.sqrt(trained.var(ddof=1) / EVAL_ENVS + rand.var(ddof=1) / EVAL_ENVS))
    print(f"snake learning: epochs={LEARN_EPOCHS} trained={trained.mean():.5f} random={rand.mean():.5f} "
          f"diff={trained.mean() - rand.mean():.5f} se={se:.5f}")
    assert trained.mean() - rand.mean() > 3 * se, (trained.mean(), rand.mean(), se)


@pytest.mark.parametrize("env_type,env_pool", [("Snake-device", None), ("Snake-host", "serial"), ("Snake-host", "process")])
def test_train_plays_the_snake_env_types(env_type, env_pool, tmp_path):
    """train() builds the pools from env_type and the reference's grid_size / unit_size / n_foods keys, without gym"""
    from a2c_amd.training import train
    hyps = dict(exp_name="snake", main_path=str(tmp_path), model="FCModel", env_type=env_type, n_envs=3, n_rollouts=3,
                n_tsteps=5, n_frame_stack=3, max_tsteps=1e9, seed=1, grid_size=[6, 6], unit_size=2, n_foods=3, h_size=32,
                n_test_eps=2, max_eval_steps=20)
    if env_pool:
        hyps["env_pool"] = env_pool
    seen = []
    best = train(None, hyps, verbose=False, max_epochs=2,
                 on_epoch=lambda epoch, upd, D: seen.append((tuple(D["states"].shape), int(D["actions"].max()))))
    assert len(seen) == 2 and seen[0][0] == (15, 3, 12, 12) and 0 <= seen[0][1] < 4
    assert np.isfinite(best)
