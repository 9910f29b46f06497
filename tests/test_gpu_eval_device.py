"""-m gpu: evaluation on the device worlds.  Env ids other than 0..B-1 on the three pools against the host twins; the
``DeviceStatsRunner`` against the twins by ACTION REPLAY (the actions the evaluator recorded, replayed on ``PongEnv`` /
``BreakoutEnv`` / ``SnakeEnv``: exact whatever the forward's last bits are); an evaluation between a rollout and its update
changes nothing; ``train()`` with ``eval_pool="device"`` steps no host twin.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import base_hyps  # noqa: E402
from test_gpu_world_post import RUNNER_B, RUNNER_CASES, RUNNER_ROUNDS, RUNNER_T, _runner  # noqa: E402

DEV = "cuda"
ID0 = 10007


def _classes(wname):
    from a2c_amd import breakout, pong, snake
    return dict(pong=(pong.DevicePongPool, pong.PongEnv), breakout=(breakout.DeviceBreakoutPool, breakout.BreakoutEnv),
                snake=(snake.DeviceSnakePool, snake.SnakeEnv))[wname]


def _twin_start(e):
    e.reset() if not hasattr(e, "new_episode") else e.new_episode()


def _twin_step(e, a):
    """-> (reward, real done); the twin is left at its reset position after a real done, as the Runner leaves the world"""
    if hasattr(e, "advance"):
        r, d = e.advance(int(a))
    else:
        _, r, d, _ = e.step(int(a))
    return float(r), bool(d)


# ---------------------------------------------------------------- env ids
ID_WORLDS = {"pong": (dict(points_to_win=2, max_episode_steps=40), 3, 1),
             "breakout": (dict(lives=1, max_episode_steps=40), 4, 2),
             "snake": (dict(grid_size=5, unit_size=4, n_foods=2), 4, 3)}
ID_STEPS, ID_B = 48, 7
PONG_WORDS = ("agent_y", "opp_y", "ball_x", "ball_y", "vx", "vy", "score_agent", "score_opp", "draws", "steps", "ep_steps")


def _twin_frame(wname, e):
    from a2c_amd import preprocessing
    if wname == "snake":
        return np.asarray(preprocessing.snake_prep(e.render_rgb())[0], dtype=np.float32).reshape(-1)
    return e.prepped().astype(np.float32).reshape(-1)


def _twin_words(wname, e):
    if wname == "pong":
        return np.array([getattr(e, k) for k in PONG_WORDS], dtype=np.int64) & 0xFFFFFFFF
    if wname == "breakout":
        return np.asarray(e.state_words(), dtype=np.int64) & 0xFFFFFFFF
    return None           # (the Snake twin keeps no word image: its raw frame shows the whole state)


@functools.lru_cache(maxsize=None)
def id_twins(wname, id0):
    """ID_B twins with env ids id0 .. on the RandomState(1234) actions, restarted after a real done -> per step rew, done
    (what device_step returns: with the Pong override), reset, frames, state words, raw frames (Snake).  Once per (world, id0)."""
    world, n_act, seed = ID_WORLDS[wname]
    acts = np.random.RandomState(1234).randint(0, n_act, size=(ID_STEPS, ID_B)).astype(np.int64)
    envs = [_classes(wname)[1](seed=seed, env_id=id0 + j, **world) for j in range(ID_B)]
    rows = []

    def row(rew=None, done=None, reset=None):
        words = [_twin_words(wname, e) for e in envs]
        rows.append(dict(rew=rew, done=done, reset=reset, frames=np.stack([_twin_frame(wname, e) for e in envs]),
                         words=None if words[0] is None else np.stack(words),
                         rgb=np.stack([e.render_rgb() for e in envs]) if wname == "snake" else None))
    for e in envs:
        _twin_start(e)
    row()
    for t in range(ID_STEPS):
        rew, done, reset = (np.zeros(ID_B, dtype=np.float32) for _ in range(3))
        for j, e in enumerate(envs):
            r, d = _twin_step(e, acts[t, j])
            rew[j], reset[j], done[j] = r, d, d or (wname == "pong" and r != 0)
            if d:
                _twin_start(e)
        row(rew, done, reset)
    return acts, rows


def _assert_pool_is(wname, pool, row, what):
    assert np.array_equal(pool.frames.cpu().numpy(), row["frames"]), (what, "frames")
    if row["words"] is not None:
        n = row["words"].shape[1]
        assert np.array_equal(pool.state[:, :n].cpu().numpy().astype(np.int64) & 0xFFFFFFFF, row["words"]), (what, "state")
    if row["rgb"] is not None:
        assert np.array_equal(pool.rgb.cpu().numpy(), row["rgb"]), (what, "raw frames")


def _id_pool(wname, **kw):
    world, _, seed = ID_WORLDS[wname]
    if wname == "snake":
        kw["raw_frames"] = True
    return _classes(wname)[0](ID_B, DEV, seed=seed, **world, **kw)


def _play_ids(wname, pool, id0):
    acts, rows = id_twins(wname, id0)
    d_acts = torch.from_numpy(acts).to(DEV)
    _assert_pool_is(wname, pool, rows[0], (wname, id0, "reset"))
    for t in range(ID_STEPS):
        fr, r, d, rs = pool.step(d_acts[t].data_ptr(), 1)
        for name, got in (("rew", r), ("done", d), ("reset", rs)):
            assert np.array_equal(got.cpu().numpy(), rows[t + 1][name]), (wname, id0, t, name)
        _assert_pool_is(wname, pool, rows[t + 1], (wname, id0, t))
    resets = sum(int(rw["reset"].sum()) for rw in rows[1:])
    assert resets >= 1 and any((rw["rew"] != 0).any() for rw in rows[1:]), "the tape shows episodes ending and rewards"


@pytest.mark.parametrize("wname", list(ID_WORLDS))
def test_pools_play_the_worlds_of_their_env_ids(wname):
    pool = _id_pool(wname, env_id0=ID0)
    (pool.reset if wname == "snake" else pool.reset_all)()
    _play_ids(wname, pool, ID0)
    # the ids matter: the same tape on ids 0.. is another game
    assert any(not np.array_equal(a["frames"], b["frames"]) for a, b in zip(id_twins(wname, ID0)[1], id_twins(wname, 0)[1]))
    # a pool re-based in place is the pool built there (after it has played elsewhere)
    (pool.reset if wname == "snake" else pool.reset_all)(env_id0=ID0 + ID_B)
    fresh = _id_pool(wname, env_id0=ID0 + ID_B)
    (fresh.reset if wname == "snake" else fresh.reset_all)()
    assert pool.env_id0 == fresh.env_id0 == ID0 + ID_B
    assert torch.equal(pool.state, fresh.state) and torch.equal(pool.frames, fresh.frames)
    _play_ids(wname, pool, ID0 + ID_B)
    _play_ids(wname, fresh, ID0 + ID_B)
    assert torch.equal(pool.state, fresh.state)
    with pytest.raises(ValueError):
        _id_pool(wname, env_id0=-1)


def test_default_env_ids_are_unchanged():
    for wname in ID_WORLDS:
        pool = _id_pool(wname)
        assert pool.env_id0 == 0
        (pool.reset if wname == "snake" else pool.reset_all)()
        _play_ids(wname, pool, 0)


# ---------------------------------------------------------------- the evaluator against the twins, by action replay
EVAL_E, EVAL_SEED = 7, 3
# model, env_type, state shape, world, kwargs of the world, actions, eval_chunk, max_eval_steps, seed of the uniforms' tape
EVAL_CASES = {
    "fc_pong": ("FCModel", "Pong-device", (4, 80, 80), "pong", dict(points_to_win=1, max_episode_steps=60), 3, 16, 200, 0),
    "grufc_pong": ("GRUFCModel", "Pong-device", (4, 80, 80), "pong", dict(points_to_win=1, max_episode_steps=60), 3, 16, 200, 0),
    "fc_pong_capped": ("FCModel", "Pong-device", (4, 80, 80), "pong", dict(points_to_win=1, max_episode_steps=60), 3, 16, 40, 0),
    "grufc_pong_capped": ("GRUFCModel", "Pong-device", (4, 80, 80), "pong", dict(points_to_win=1, max_episode_steps=60), 3, 16,
                          40, 0),
    "a3c_breakout": ("A3CModel", "Breakout-device", (4, 80, 72), "breakout", dict(lives=1), 4, 32, 100, 5),
    "a3c_snake": ("A3CModel", "Snake-device", (4, 84, 84), "snake", dict(grid_size=21, unit_size=4, n_foods=2), 4, 4, 40, 71),
}


def _evaluator(case, net_seed=5, tape_seed=None, keep_actions=True):
    import a2c_amd
    from a2c_amd.runner import DeviceStatsRunner
    kind, env_type, ss, wname, world, n_act, chunk, cap, tseed = EVAL_CASES[case]
    hyps = base_hyps(env_type=env_type, n_test_eps=EVAL_E, eval_chunk=chunk, max_eval_steps=cap)
    torch.manual_seed(net_seed)
    net = getattr(a2c_amd.models, kind)(list(ss), n_act, h_size=64 if "FC" in kind else 256, bnorm=False)
    g = torch.Generator().manual_seed(tseed if tape_seed is None else tape_seed)
    steps = -(-cap // chunk) * chunk
    us, call = torch.rand((2, steps, EVAL_E), generator=g).to(DEV), [0]
    pool = _classes(wname)[0](EVAL_E, DEV, seed=EVAL_SEED, **world)
    ev = DeviceStatsRunner(hyps, pool, uniform_fn=lambda t, Bn, env0: us[call[0], t, env0:env0 + Bn].contiguous(),
                           keep_actions=keep_actions)
    return net, ev, call


def replay(case, call, last):
    """the recorded actions of one evaluation on the host twins -> ep_rew (fp32, summed step by step), ep_len, active; the
    recorded rewards / dones rows are compared on the way, up to each env's end"""
    _, _, _, wname, world, _, _, cap, _ = EVAL_CASES[case]
    pong = wname == "pong"
    acts, rews, dones = (last[k].numpy() for k in ("actions", "rewards", "dones"))
    ep_rew, ep_len, active = np.zeros(EVAL_E, dtype=np.float32), np.zeros(EVAL_E, dtype=np.int32), np.ones(EVAL_E, dtype=np.int32)
    for j in range(EVAL_E):
        e = _classes(wname)[1](seed=EVAL_SEED, env_id=ID0 + call * EVAL_E + j, **world)
        _twin_start(e)
        for t in range(cap):
            assert t < acts.shape[0], "the evaluator stopped while this env was playing"
            r, d = _twin_step(e, acts[t, j])
            done = d or (pong and r != 0)                    # the Pong override (runner.py:213-214)
            assert rews[t, j] == r and dones[t, j] == float(done), (case, call, j, t)
            ep_rew[j] = np.float32(ep_rew[j] + np.float32(r))
            ep_len[j] += 1
            if done:
                active[j] = 0
                break
    return ep_rew, ep_len, active


@pytest.mark.parametrize("case", list(EVAL_CASES))
def test_evaluator_equals_the_replay_on_the_host_twins(case):
    _, _, _, wname, _, n_act, chunk, cap, _ = EVAL_CASES[case]
    net, ev, call = _evaluator(case)
    seen = []
    for call[0] in range(2):
        got = ev.rollout(net)
        last = ev.last
        ep_rew, ep_len, active = replay(case, call[0], last)
        print(f"{case} call {call[0]}: ep_len {ep_len.tolist()} ep_rew {ep_rew.tolist()} active {active.tolist()} "
              f"steps {last['steps']} chunks {last['chunks']} "
              f"actions {np.bincount(last['actions'].numpy().reshape(-1), minlength=n_act)}")
        assert np.array_equal(last["ep_rew"].numpy(), ep_rew) and last["ep_rew"].dtype == torch.float32
        assert np.array_equal(last["ep_len"].numpy(), ep_len) and np.array_equal(last["active"].numpy(), active)
        assert got == float(ep_rew.astype(np.float64).sum()) / EVAL_E
        assert last["actions"].shape == (last["steps"], EVAL_E) and last["actions"].dtype == torch.int64
        assert last["steps"] == min(last["chunks"] * chunk, cap)
        # the loop stopped where it had to: not before the last env's end, and in that env's chunk (or at the cap)
        longest = int(ep_len.max())
        assert last["chunks"] == -(-(cap if active.any() else longest) // chunk)
        # what the case is there to show, on the replay
        assert (active == 0).any(), "an env ended before the cap"
        assert len(set(ep_len.tolist())) >= 2, "two different episode lengths"
        if wname != "snake":
            assert (ep_rew != 0).any(), "a nonzero episode reward"
        if case.endswith("_capped") or case == "a3c_breakout":
            assert (active != 0).any() and int(ep_len[active != 0].min()) == cap, "an env played on to the cap"
        assert last["chunks"] >= 3
        # chunk 0 eager, chunk 1 captured, the rest replays: one graph, whatever the call
        graphs = list(ev.runner._dev_graphs.values())
        assert len(graphs) == 1 and isinstance(graphs[0], torch.cuda.CUDAGraph), graphs
        seen.append((ep_len.tolist(), last["actions"].clone()))
    assert ev.pool.env_id0 == ID0 + EVAL_E and ev.calls == 2
    assert seen[0][0] != seen[1][0] or not torch.equal(seen[0][1], seen[1][1]), "the second call played other worlds"


def test_evaluations_are_reproducible():
    """a second evaluator with the same tape plays the same two evaluations: the worlds of a call depend on the call alone"""
    out = []
    for _ in range(2):
        net, ev, call = _evaluator("fc_pong_capped")
        res = []
        for call[0] in range(2):
            res.append((ev.rollout(net), ev.last["actions"].clone(), ev.last["ep_len"].clone()))
        out.append(res)
    for a, b in zip(*out):
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_evaluator_refuses_what_it_cannot_play():
    from a2c_amd.runner import DeviceStatsRunner, HostEnvPool
    with pytest.raises(ValueError):
        DeviceStatsRunner(base_hyps(), HostEnvPool([], frame_shape=(1, 4, 4)))
    pool = _classes("pong")[0](2, DEV)
    with pytest.raises(ValueError):
        DeviceStatsRunner(base_hyps(eval_chunk=-1), pool)


# ---------------------------------------------------------------- non-interference
def _train_rounds(case, evaluate):
    from a2c_amd.runner import DeviceStatsRunner
    from a2c_amd.updater import Updater
    g = torch.Generator().manual_seed(3)
    us, rnd = torch.rand((RUNNER_ROUNDS, RUNNER_T, RUNNER_B), generator=g).to(DEV), [0]
    net, D, pool, hyps, r = _runner(case, True, lambda t, Bn, env0: us[rnd[0], t, env0:env0 + Bn].contiguous())
    upd = Updater(net, hyps)
    ev, scores = None, []
    if evaluate:
        _, _, _, wname, world, _ = RUNNER_CASES[case]
        ge = torch.Generator().manual_seed(17)
        ue = torch.rand((RUNNER_ROUNDS, 12, 3), generator=ge).to(DEV)
        ev = DeviceStatsRunner(dict(hyps, eval_chunk=4, max_eval_steps=12), _classes(wname)[0](3, DEV, seed=12, **world),
                               uniform_fn=lambda t, Bn, env0: ue[rnd[0], t, env0:env0 + Bn].contiguous())
    rows = []
    for rnd[0] in range(RUNNER_ROUNDS):
        r.rollout(net, list(range(RUNNER_B)), hyps)
        r.finish()
        rows.append({k: v.clone() for k, v in D.items()})
        route = net._route_sig()
        if ev is not None:
            scores.append((ev.rollout(net), ev.last["steps"]))
            assert net._route_sig() == route, "what the rollout left in the net for its update"
        upd.update_model(D)
    torch.cuda.synchronize()
    return rows, [p.detach().clone() for p in net.parameters()], scores, route


@pytest.mark.parametrize("case", ["fc_pong", "a3c_snake"])
def test_an_evaluation_between_rollout_and_update_changes_nothing(case):
    want, params_w, _, route = _train_rounds(case, False)
    got, params, scores, _ = _train_rounds(case, True)
    print(f"{case}: evaluations {scores}, stash {route[0]}")
    assert len(scores) == RUNNER_ROUNDS and all(s[1] >= 1 for s in scores)
    if case == "a3c_snake":
        assert route[0] is not None, "the step kernel stashed activations for the update"
    for k in range(RUNNER_ROUNDS):
        for name in want[k]:
            assert torch.equal(got[k][name], want[k][name]), (case, k, name)
    for p, q in zip(params, params_w):
        assert torch.equal(p, q)
    assert not torch.equal(want[0]["states"], want[-1]["states"])


# ---------------------------------------------------------------- train()
def test_train_eval_pool_device_steps_no_host_twin(tmp_path, monkeypatch):
    from a2c_amd import pong
    from a2c_amd.training import train
    g = torch.Generator().manual_seed(21)
    us = torch.rand((12, RUNNER_B), generator=g).to(DEV)
    params, best = {}, {}

    def run(eval_pool):
        hyps = dict(exp_name=f"pong_{eval_pool}", main_path=str(tmp_path), model="FCModel", env_type="Pong-device",
                    n_envs=RUNNER_B, n_rollouts=RUNNER_B, n_tsteps=RUNNER_T, n_frame_stack=3, max_tsteps=1e9, seed=1,
                    points_to_win=1, max_episode_steps=10, h_size=32, n_test_eps=2, eval_chunk=4, max_eval_steps=12,
                    eval_pool=eval_pool)
        torch.manual_seed(3)
        best[eval_pool] = train(None, hyps, verbose=False, max_epochs=3, uniform_fn=lambda t, Bn, env0=0: us[t, env0:env0 + Bn],
                                on_epoch=lambda epoch, upd, D: params.setdefault(eval_pool, []).append(
                                    [p.detach().clone() for p in upd.net.parameters()]))
    run("host")

    def no_step(self, action):
        raise AssertionError("a host twin was stepped")
    monkeypatch.setattr(pong.PongEnv, "step", no_step)
    run("device")
    assert np.isfinite(best["device"]) and -1.0 <= best["device"] <= 1.0
    assert len(params["device"]) == 3 and len(params["host"]) == 3
    for p, q in zip(params["device"][-1], params["host"][-1]):
        assert torch.equal(p, q)
    assert not torch.equal(params["device"][0][0], params["device"][-1][0])
    # ... the patch is what the first assertion rests on: the twins train() builds for the host evaluation step through it
    from a2c_amd import preprocessing
    from a2c_amd.runner import SequentialEnvironment
    twin = SequentialEnvironment("Pong-device", preprocessing.pong_prep, seed=1, env_fn=pong.PongFactory(env_id=ID0, seed=1))
    with pytest.raises(AssertionError, match="host twin"):
        twin.step(0)
