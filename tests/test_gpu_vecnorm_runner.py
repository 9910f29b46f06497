"""-m gpu: running normalisation through the Runner (hyps norm_obs / norm_rewards): rollouts on the device
pools of the three vector worlds replayed through host twins and a ``RunningNorm``; the graph path against the eager loop;
nothing without the keys; evaluation on the device against lock-step host twins; ``train()`` and its checkpoints.  The worlds
are integers and the normaliser's arithmetic has a fixed order, so every comparison is bit equality."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import base_hyps  # noqa: E402
from test_gpu_pendulum import _CountedLib  # noqa: E402
from test_pendulum import CAP, REPEAT  # noqa: E402

DEV = "cuda"
B, T, C, ROUNDS = 8, 8, 4, 5
GAMMA = 0.99
KINDS = ("FCModel", "GRUFCModel")


def _world(family):
    """-> (device pool class, host twin class, world keywords, L, action size, continuous)"""
    from a2c_amd import cartpole, pendulum, point
    if family == "Pendulum":
        return pendulum.DevicePendulumPool, pendulum.PendulumEnv, dict(max_episode_steps=CAP), 4, 1, True
    if family == "CartPole":
        return cartpole.DeviceCartPolePool, cartpole.CartPoleEnv, dict(max_episode_steps=CAP), 4, 2, False
    return point.DevicePointPool, point.PointEnv, dict(max_episode_steps=CAP, targets_to_win=2), 8, 2, True


def _net(kind, L, n_act, cont, seed=5):
    import a2c_amd
    torch.manual_seed(seed)
    return getattr(a2c_amd.models, kind)([C, L], n_act, h_size=32, bnorm=False, is_discrete=not cont)


def _datas(net, L, n_act, cont, N=B * T):
    D = dict(states=torch.zeros(N, C, L, device=DEV), deltas=torch.zeros(N, device=DEV), rewards=torch.zeros(N, device=DEV),
             dones=torch.zeros(N, device=DEV),
             actions=torch.zeros(N, n_act, device=DEV) if cont else torch.zeros(N, dtype=torch.int64, device=DEV))
    if net.is_recurrent:
        D["h_states"] = torch.zeros(N, net.h_size, device=DEV)
    return D


def _hyps(family, cont, **kw):
    return base_hyps(**dict(dict(env_type=family + "-device", n_tsteps=T, n_rollouts=B, n_envs=B, n_frame_stack=C,
                                 is_discrete=not cont, h_size=32, gamma=GAMMA, norm_obs=True, norm_rewards=True), **kw))


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    bad = got.view(np.int32) != want.view(np.int32)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        print(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {i}: got {got[i]!r}, want {want[i]!r}")
    assert not bad.any(), what


def _replay(family, kind, norm_obs=True, norm_rewards=True):
    """ROUNDS rollouts of the eager loop with the values of every forward kept; the recorded actions replayed through host
    twins and a RunningNorm -> what the rows must hold"""
    from a2c_amd.runner import Runner
    from a2c_amd.vecnorm import RunningNorm
    pool_cls, env_cls, world, L, n_act, cont = _world(family)
    hyps = _hyps(family, cont, rollout_graphs=False, norm_obs=norm_obs, norm_rewards=norm_rewards, norm_clip_obs=2.0,
                 norm_clip_rew=1.5)
    net = _net(kind, L, n_act, cont)
    D = _datas(net, L, n_act, cont)
    r = Runner(D, hyps, None, None, None, env_pool=pool_cls(B, DEV, seed=12, **world))
    vals, fwd = [], r._forward

    def keep(*a, **k):
        out = fwd(*a, **k)
        vals.append(out["vals"].clone())
        return out
    r._forward = keep
    envs = [env_cls(seed=12, env_id=j, **world) for j in range(B)]
    tw = RunningNorm(L, B, GAMMA, clip_obs=2.0, clip_rew=1.5)
    obs = np.stack([np.asarray(e.reset(), dtype=np.float32).reshape(L) for e in envs])
    if norm_obs:
        obs, _ = tw.step(obs, None, None, 0)
    state = np.zeros((B, C, L), dtype=np.float32)
    state[:, C - 1] = obs
    g32 = np.float32(GAMMA)
    closed = clipped = 0
    for rnd in range(ROUNDS):
        del vals[:]
        r.rollout(net, list(range(B)), hyps)
        r.finish()
        got = {k: v.cpu().numpy() for k, v in D.items()}
        v = torch.stack(vals).cpu().numpy()                       # (T + 1, B): the T states and the bootstrap
        assert v.shape == (T + 1, B)
        acts = got["actions"].reshape(B, T, -1)
        want_s, want_r, want_d = (np.zeros((B, T) + s, dtype=np.float32) for s in ((C, L), (), ()))
        for t in range(T):
            want_s[:, t] = state
            new, rew, done = np.zeros((B, L), np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)
            for j, e in enumerate(envs):
                o, rew[j], d, _ = e.step(acts[j, t] if cont else int(acts[j, t, 0]))
                done[j] = float(d)
                new[j] = np.asarray(e.reset() if d else o, dtype=np.float32).reshape(L)
            closed += int(done.sum())
            o_n, r_n = tw.step(new if norm_obs else None, rew if norm_rewards else None, done if norm_rewards else None, 0)
            new, rew = (new if o_n is None else o_n), (rew if r_n is None else r_n)
            clipped += int((np.abs(new) == 2.0).sum()) + int((np.abs(rew) == 1.5).sum())
            nxt = np.zeros_like(state)
            nxt[:, :C - 1] = np.where(done[:, None, None] != 0, 0.0, state[:, 1:])
            nxt[:, C - 1] = new
            state = nxt
            want_r[:, t], want_d[:, t] = rew, done
        # the bootstrap closes the slot: the last reward takes gamma * V(bookmark) where the step did not close
        opened = want_d[:, T - 1] == 0
        want_r[:, T - 1] = np.where(opened, want_r[:, T - 1] + g32 * v[T], want_r[:, T - 1])
        want_d[:, T - 1] = 1.0
        _bits_equal(got["states"].reshape(B, T, C, L), want_s, f"{family} {kind} round {rnd}: states")
        _bits_equal(got["rewards"].reshape(B, T), want_r, f"{family} {kind} round {rnd}: rewards")
        _bits_equal(got["dones"].reshape(B, T), want_d, f"{family} {kind} round {rnd}: dones")
        _bits_equal(r.bookmark.cpu().numpy().reshape(B, C, L), state, f"{family} {kind} round {rnd}: bookmark")
        # a2c_td_delta in fp32 from the recorded rows and the values: r + (gamma * v') * (1 - d) - v, every operation rounded
        rw, dn = got["rewards"].reshape(B, T), got["dones"].reshape(B, T)
        want_delta = np.zeros((B, T), dtype=np.float32)
        for t in range(T - 1):
            want_delta[:, t] = (rw[:, t] + (g32 * v[t + 1]) * (np.float32(1) - dn[:, t])) - v[t]
        want_delta[:, T - 1] = rw[:, T - 1] - v[T - 1]
        _bits_equal(got["deltas"].reshape(B, T), want_delta, f"{family} {kind} round {rnd}: deltas")
        blk = r.vecnorm.block.cpu().numpy()
        assert blk.tobytes() == tw.to_block().tobytes(), f"{family} {kind} round {rnd}: the block"
    print(f"vecnorm runner {family} {kind} obs={norm_obs} rew={norm_rewards}: closed {closed}, at a clip {clipped}, "
          f"counts {blk[0]}, {blk[1 + 2 * L]}")
    assert closed >= B, "episodes end inside the rollouts"
    return r, tw, clipped


@pytest.mark.parametrize("kind", KINDS)
def test_pendulum_rollouts_equal_the_replay(kind):
    r, tw, clipped = _replay("Pendulum", kind)
    assert clipped > 0 and tw.obs_count == pytest.approx(1e-4 + B * (1 + ROUNDS * T), rel=1e-12)
    assert tw.ret_count == pytest.approx(1e-4 + B * ROUNDS * T, rel=1e-12)
    # the pool's own reward row and its episode sums stay the game's: integers times 2^-8, the floored sums whole units
    raw = r.env_pool.rew.cpu().numpy() * 256
    assert (raw == np.round(raw)).all() and (raw < 0).any()


@pytest.mark.parametrize("family,kind", [("CartPole", "FCModel"), ("Point", "GRUFCModel")])
def test_cartpole_and_point_rollouts_equal_the_replay(family, kind):
    _replay(family, kind)


@pytest.mark.parametrize("norm_obs,norm_rewards", [(True, False), (False, True)])
def test_either_key_alone(norm_obs, norm_rewards):
    r, tw, _ = _replay("Pendulum", "FCModel", norm_obs=norm_obs, norm_rewards=norm_rewards)
    assert (tw.obs_count == 1e-4) == (not norm_obs) and (tw.ret_count == 1e-4) == (not norm_rewards)


# ---------------------------------------------------------------- the graph path against the eager loop
def _play(kind, graphs, keys=True):
    """ROUNDS rollouts (eager, captured, replayed x 3 on the graph path), an update after each"""
    from a2c_amd import ops
    from a2c_amd.pendulum import DevicePendulumPool
    from a2c_amd.runner import Runner
    from a2c_amd.updater import Updater
    g = torch.Generator().manual_seed(4)
    eps, rnd = (3.0 * torch.randn((ROUNDS, T, B, 1), generator=g)).to(DEV), [0]
    hyps = _hyps("Pendulum", True, rollout_graphs=graphs, action_shift=0.5, norm_obs=keys, norm_rewards=keys)
    if not keys:
        del hyps["norm_obs"], hyps["norm_rewards"]
    net = _net(kind, 4, 1, True)
    D = _datas(net, 4, 1, True)
    pool = DevicePendulumPool(B, DEV, seed=12, max_episode_steps=CAP, **REPEAT)
    r = Runner(D, hyps, None, None, None, env_pool=pool, normal_fn=lambda t, Bn, env0: eps[rnd[0], t, env0:env0 + Bn])
    upd = Updater(net, hyps)
    rows, launches, names = [], [], set()
    for rnd[0] in range(ROUNDS):
        real, counted = ops.lib, _NamedLib(ops.lib(), names)
        ops.lib = lambda: counted
        try:
            r.rollout(net, list(range(B)), hyps)
        finally:
            ops.lib = real
        r.finish()
        launches.append(counted.n)
        rows.append({k: v.clone() for k, v in D.items()})
        upd.update_model(D)
    torch.cuda.synchronize()
    return dict(rows=rows, state=pool.state.clone(), stats=pool.ep_stats.clone(), runner=r, names=names,
                params=[p.detach().clone() for p in net.parameters()], graphs=list(r._dev_graphs.values()), launches=launches,
                block=None if r.vecnorm is None else r.vecnorm.block.clone())


class _NamedLib(_CountedLib):
    """... and the names of the entry points called"""

    def __init__(self, lib, names):
        super().__init__(lib)
        self._names = names

    def __getattr__(self, name):
        if name.startswith("a2c_"):
            self._names.add(name)
        return super().__getattr__(name)


@pytest.mark.parametrize("kind", KINDS)
def test_graph_path_equals_the_eager_loop(kind):
    got, want = _play(kind, True), _play(kind, False)
    n, n_w = got["launches"], want["launches"]
    print(f"vecnorm pendulum {kind}: launches per rollout, graph path {n}, eager {n_w}")
    assert len(got["graphs"]) == 1 and isinstance(got["graphs"][0], torch.cuda.CUDAGraph) and not want["graphs"]
    assert n[0] > 0 and n[1] > 0 and n[2:] == [0, 0, 0] and min(n_w) > 0, "a replayed rollout is the replay and nothing else"
    assert "a2c_vecnorm_step" in got["names"] and "a2c_vecnorm_step" in want["names"]
    for k in range(ROUNDS):
        for name in want["rows"][k]:
            assert torch.equal(got["rows"][k][name], want["rows"][k][name]), (kind, k, name)
    assert torch.equal(got["state"], want["state"]) and torch.equal(got["stats"], want["stats"])
    assert torch.equal(got["block"].view(torch.int64), want["block"].view(torch.int64))
    for p, q in zip(got["params"], want["params"]):
        assert torch.equal(p, q)
    # the replays advanced the block: every step of every rollout was counted, and the first observation
    count = rcount = np.float64(1e-4)
    for k in range(1 + ROUNDS * T):
        count = count + np.float64(B)
        rcount = rcount + np.float64(B) if k else rcount
    assert float(got["block"][0]) == count and float(got["block"][1 + 2 * 4]) == rcount
    assert int(want["stats"][0]) >= B, "episodes end inside the rollouts"


def test_without_the_keys_nothing_is_launched_or_allocated():
    got = _play("FCModel", True, keys=False)
    assert got["runner"].vecnorm is None and got["block"] is None
    assert "a2c_vecnorm_step" not in got["names"] and "a2c_vecnorm_init" not in got["names"]
    assert "a2c_pendulum_step" in got["names"]
    on = _play("FCModel", True, keys=True)
    assert not torch.equal(on["rows"][0]["rewards"], got["rows"][0]["rewards"])
    # (round 1 is the capture: every launch of the slot is issued once, and start() is behind)
    assert on["launches"][1] == got["launches"][1] + T, "one launch per env step is what the keys add"


def test_runner_refuses_what_the_normaliser_does_not_cover():
    import a2c_amd
    from a2c_amd.pendulum import PendulumEnv
    from a2c_amd.pong import DevicePongPool
    from a2c_amd.runner import DeviceStatsRunner, HostEnvPool, Runner, StatsRunner
    net = _net("FCModel", 4, 1, True)
    D = _datas(net, 4, 1, True)
    hyps = _hyps("Pendulum", True)
    host = HostEnvPool([PendulumEnv(seed=1, env_id=j) for j in range(B)], frame_shape=(1, 4))
    with pytest.raises(ValueError, match="norm_obs"):
        Runner(D, hyps, None, None, None, env_pool=host).start(net)
    with pytest.raises(ValueError, match="norm_rewards"):
        Runner(D, dict(hyps, norm_obs=False), None, None, None, env_pool=host).start(net)
    pix = a2c_amd.models.FCModel([C, 80, 72], 3, h_size=32, bnorm=False)
    with pytest.raises(ValueError, match="norm_obs"):
        Runner(D, dict(hyps, env_type="Pong-device", is_discrete=True), None, None, None,
               env_pool=DevicePongPool(B, DEV)).start(pix)
    with pytest.raises(ValueError, match="norm_obs"):
        DeviceStatsRunner(hyps, _world("Pendulum")[0](2, DEV))
    with pytest.raises(ValueError, match="norm_obs"):
        StatsRunner(hyps, envs=[PendulumEnv()])


# ---------------------------------------------------------------- evaluation
@pytest.mark.parametrize("kind", KINDS)
def test_device_evaluation_equals_host_twins_and_leaves_the_block(kind):
    """a block trained for two rollouts with an update each; E episodes on the device (frozen mode) against StatsRunner's
    lock-step loop over host twins normalised by one snapshot()"""
    from a2c_amd.pendulum import DevicePendulumPool, PendulumEnv
    from a2c_amd.runner import DeviceStatsRunner, Runner, StatsRunner
    from a2c_amd.updater import Updater
    E, K, cap = 6, 8, 20
    hyps = _hyps("Pendulum", True, n_test_eps=E, eval_chunk=K, max_eval_steps=cap, action_shift=0.5)
    net = _net(kind, 4, 1, True)
    D = _datas(net, 4, 1, True)
    r = Runner(D, hyps, None, None, None, env_pool=DevicePendulumPool(B, DEV, seed=12, max_episode_steps=CAP))
    upd = Updater(net, hyps)
    for _ in range(2):
        r.rollout(net, list(range(B)), hyps)
        r.finish()
        upd.update_model(D)
    block0 = r.vecnorm.block.clone()
    assert float(block0[0]) > 100 and float(block0[1:5].abs().max()) > 0
    g = torch.Generator().manual_seed(9)
    eps = (3.0 * torch.randn((2 * cap, E, 1), generator=g)).to(DEV)
    fn = lambda t, En, env0: eps[t, env0:env0 + En]
    world = dict(max_episode_steps=13)
    dsr = DeviceStatsRunner(hyps, DevicePendulumPool(E, DEV, seed=4, **world), normal_fn=fn, keep_actions=True, norm=r.vecnorm)
    plain = DeviceStatsRunner(dict(hyps, norm_obs=False), DevicePendulumPool(E, DEV, seed=4, **world), normal_fn=fn)
    for call in range(2):
        twins = [PendulumEnv(seed=4, env_id=10007 + call * E + j, **world) for j in range(E)]
        got = dsr.rollout(net)
        want = StatsRunner(hyps, envs=twins, normal_fn=fn, norm=lambda: r.vecnorm).rollout(net)
        raw = plain.rollout(net)
        print(f"vecnorm eval {kind} call {call}: device {got}, host twins {want}, unnormalised {raw}")
        assert got == want and got < 0
        # the same worlds, net and noise without the block play another game: what the net saw was normalised
        assert got != raw and not torch.equal(dsr.datas["states"], plain.datas["states"])
        frac = dsr.last["ep_rew"].double() * 256
        assert torch.equal(frac, frac.round()), "an evaluation return is the game's: rewards are not normalised"
        assert dsr.last["ep_len"].tolist() == [13] * E
    assert dsr.runner.vecnorm is r.vecnorm and plain.runner.vecnorm is None
    assert torch.equal(r.vecnorm.block.view(torch.int64), block0.view(torch.int64)), "the block is bit-unchanged by both"


# ---------------------------------------------------------------- train()
def _train_hyps(tmp_path, **kw):
    return dict(dict(exp_name="vn", main_path=str(tmp_path), model="FCModel", env_type="Pendulum-device", n_envs=8, n_rollouts=8,
                     n_tsteps=8, n_frame_stack=3, max_tsteps=1e9, seed=1, max_episode_steps=CAP, h_size=32, n_test_eps=2,
                     max_eval_steps=20, norm_obs=True, norm_rewards=True), **kw)


@pytest.mark.parametrize("eval_pool", ["host", "device"])
def test_train_writes_norm_p_and_a_resumed_run_loads_it(eval_pool, tmp_path, monkeypatch):
    from a2c_amd.training import train
    from a2c_amd.vecnorm import DeviceVecNorm, RunningNorm
    seen = []
    best = train(None, _train_hyps(tmp_path, eval_pool=eval_pool), verbose=False, max_epochs=2,
                 on_epoch=lambda epoch, upd, D: seen.append((float(D["rewards"].view(8, 8)[:, :-1].abs().max()),
                                                             float(D["states"].abs().max()))))
    folder = os.path.join(str(tmp_path), "vn", "vn_0")
    assert np.isfinite(best) and best < 0 and len(seen) == 2
    assert seen[0][0] <= 10.0 and seen[0][1] <= 10.0, "what the update saw was clipped at 10"
    for name in ("norm.p", "best_norm.p", "net.p", "optim.p", "best_net.p"):
        assert os.path.exists(os.path.join(folder, name)), name
    sd = torch.load(os.path.join(folder, "norm.p"))
    first = RunningNorm(4, 8, 0.99).load_state_dict(sd)
    def count(c, launches):               # the kernel's count: one addition of the 8 envs per launch
        for _ in range(launches):
            c = c + np.float64(8)
        return c
    # the first observation and two collected epochs of 8 steps; the returns have no first observation
    assert first.obs_count == count(np.float64(1e-4), 1 + 2 * 8) and first.ret_count == count(np.float64(1e-4), 2 * 8)
    assert first.obs_var[3] < 1e-4 and first.obs_mean[3] == 0.0 and first.ret_var > 1.0
    # bit for bit into a device block ...
    dv = DeviceVecNorm(4, 8, 0.5, device=DEV).load_state_dict(sd)
    assert dv.block.cpu().numpy().tobytes() == first.to_block().tobytes() and dv.gamma == first.gamma
    # ... and a resumed run starts from it: its own first observation and one epoch on top of the loaded counts.  (train()
    # numbers a new folder for every run, a resumed one included; the run is pointed at the folder that holds the checkpoints)
    from a2c_amd import training
    monkeypatch.setattr(training, "get_exp_num", lambda main_path, exp_name: 0)
    loads, real_load = [], DeviceVecNorm.load

    def load(self, norm):
        """what the resumed run's rollout thread hands its block, and the block before and after"""
        before = self.block.cpu().numpy().copy()
        out = real_load(self, norm)
        given = norm if not isinstance(norm, dict) else RunningNorm(4, 8, 0.5).load_state_dict(norm)
        loads.append((before, given.to_block(), self.block.cpu().numpy().copy()))
        return out
    monkeypatch.setattr(DeviceVecNorm, "load", load)
    train(None, dict(_train_hyps(tmp_path, eval_pool=eval_pool), resume=True), verbose=False, max_epochs=1)
    monkeypatch.setattr(DeviceVecNorm, "load", real_load)
    assert len(loads) == 1, "one load: the training Runner's block, in start()"
    before, given, after = loads[0]
    saved = first.to_block().tobytes()
    assert given.tobytes() == saved and after.tobytes() == saved, "norm.p reaches the block bit for bit"
    # ... before anything was folded in: the block it replaced was a fresh one, and the first observation came on top
    assert before.tobytes() == RunningNorm(4, 8, 0.99).to_block().tobytes()
    again = RunningNorm(4, 8, 0.99).load_state_dict(torch.load(os.path.join(folder, "norm.p")))
    assert again.obs_count == count(first.obs_count, 1 + 8) and again.ret_count == count(first.ret_count, 8)
    assert again.to_block().tobytes() != saved


@pytest.mark.parametrize("kw,key", [(dict(env_type="Pendulum-host", env_pool="serial"), "norm_obs"),
                                    (dict(env_type="Breakout-device", model="A3CModel"), "norm_obs"),
                                    # both are wrong here: the evaluation pool is checked first and its message wins
                                    (dict(eval_pool="device", env_type="Pendulum-host", env_pool="serial"), "eval_pool"),
                                    (dict(eval_pool="device", env_type="Breakout-device", model="A3CModel",
                                          norm_obs=False), "norm_rewards")])
def test_train_refusals(kw, key, tmp_path):
    from a2c_amd.training import train
    with pytest.raises(ValueError, match=key):
        train(None, _train_hyps(tmp_path, **kw), verbose=False, max_epochs=1)
    assert not list(tmp_path.iterdir()), "nothing was written"


def test_train_refuses_a_single_eval_env(tmp_path):
    from a2c_amd.pendulum import PendulumEnv
    from a2c_amd.training import train
    with pytest.raises(ValueError, match="norm_obs"):
        train(None, _train_hyps(tmp_path), verbose=False, max_epochs=1, eval_env=PendulumEnv())
    assert not list(tmp_path.iterdir())
