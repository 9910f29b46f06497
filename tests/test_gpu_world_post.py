"""-m gpu: a2c_<world>_step_post (world step + bookkeeping + frame stack in one launch) against the launch sequence it
replaces -- bit for bit --, its argument checks, and the Runner's one-graph device slot against ``rollout_graphs=False``:
eager, captured and replayed rollouts, with updates in between, under a caller's own capture, and through ``train()``.
Everything compared here is produced by the same arithmetic on both sides, so every comparison is ``torch.equal``."""
import ctypes
import functools
import queue

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import base_hyps  # noqa: E402

DEV = "cuda"
N_STEPS, T = 48, 3
GAMMA = 0.99
# world -> (pool kwargs, number of actions, the Runner's pong flag, seed of the worlds)
WORLDS = {"pong": (dict(points_to_win=2, max_episode_steps=40), 3, True, 1),
          "breakout": (dict(lives=1, max_episode_steps=40), 4, False, 2),
          "snake": (dict(grid_size=5, unit_size=4, n_foods=2), 4, False, 3)}
TWIN_SEEDS = (1, 2, 3)


def action_stream(wname, B):
    return np.random.RandomState(1234).randint(0, WORLDS[wname][1], size=(N_STEPS, B)).astype(np.int64)


def _pool(wname, B, seed=None):
    from a2c_amd.breakout import DeviceBreakoutPool
    from a2c_amd.pong import DevicePongPool
    from a2c_amd.snake import DeviceSnakePool
    kw, _, _, s = WORLDS[wname]
    pool = dict(pong=DevicePongPool, breakout=DeviceBreakoutPool, snake=DeviceSnakePool)[wname](
        B, DEV, seed=s if seed is None else seed, **kw)
    (pool.reset if wname == "snake" else pool.reset_all)()
    return pool


@functools.lru_cache(maxsize=None)
def twin_events(wname, seed, B=7):
    """the action stream on B host twins, restarted after a real done as the Runner does -> per env: real episode ends; per
    world: dones without a reset (only the "Pong" override makes any: a point that does not end the episode) and non-zero
    rewards on steps without a real done.  Computed once per (world, seed)."""
    from a2c_amd.breakout import BreakoutEnv
    from a2c_amd.pong import PongEnv
    from a2c_amd.snake import SnakeEnv
    kw, _, pong, _ = WORLDS[wname]
    acts = action_stream(wname, B)
    envs = [dict(pong=PongEnv, breakout=BreakoutEnv, snake=SnakeEnv)[wname](seed=seed, env_id=j, **kw) for j in range(B)]
    resets, done_only, rew_only = np.zeros(B, dtype=int), 0, 0
    for e in envs:
        e.reset() if wname == "snake" else e.new_episode()
    for t in range(N_STEPS):
        for j, e in enumerate(envs):
            if wname == "snake":
                _, r, reset, _ = e.step(int(acts[t, j]))
            else:
                r, reset = e.advance(int(acts[t, j]))
            done = reset or (pong and r != 0)          # what the Runner records (runner.py:212-214)
            resets[j] += int(reset)
            done_only += int(done and not reset)
            rew_only += int(r != 0 and not reset)
            if reset:
                e.reset() if wname == "snake" else e.new_episode()
    return resets, done_only, rew_only


def assert_the_action_stream_shows_every_event(wname):
    """a run without events cannot pass the comparison: on the host twins, with each of the seeds, every env ends at least
    one episode, every world pays a reward on a step that ends none, and Pong has dones without a reset"""
    for seed in TWIN_SEEDS:
        resets, done_only, rew_only = twin_events(wname, seed)
        print(f"{wname} twins, seed {seed}: resets per env {resets.tolist()}, dones without a reset {done_only}, "
              f"rewards without a real done {rew_only}")
        assert (resets >= 1).all(), (wname, seed, resets)
        assert rew_only >= 1, (wname, seed)
        assert done_only >= 1 if wname == "pong" else done_only == 0, (wname, seed, done_only)


class _Side:
    """one pool and one set of rollout buffers, rows addressed as in the Runner's buffers: slot0 + b, T rows per slot"""

    def __init__(self, wname, B, C, recurrent):
        self.wname, self.B, self.C = wname, B, C
        self.pool = _pool(wname, B)
        self.HW = self.pool.HW
        self.S = C * self.HW
        self.slot0 = 2
        N = (self.slot0 + B) * T
        f32 = dict(dtype=torch.float32, device=DEV)
        self.states = torch.zeros((N, self.S), **f32)
        self.bookmark = torch.zeros((B, self.S), **f32)
        ones = torch.ones(B, **f32)
        from a2c_amd import ops
        ops.frame_stack_push(self.pool.frames, ones, self.bookmark.data_ptr(), self.S, self.bookmark.data_ptr(), self.S, B, C,
                             self.HW)
        self.rewards, self.dones, self.deltas = (torch.full((N,), -7.0, **f32) for _ in range(3))
        self.val_prev, self.done_eff = torch.zeros(B, **f32), torch.full((B,), -7.0, **f32)
        self.h = torch.zeros((B, 5), **f32) if recurrent else None

    def sp(self, t):
        return self.states.data_ptr() + 4 * (self.slot0 * T + t) * self.S

    def rows(self, t):
        if t + 1 < T:
            return self.sp(t + 1), T * self.S
        return self.bookmark.data_ptr(), self.S

    def tensors(self, frames=True):
        p = self.pool
        out = dict(state=p.state, rew=p.rew, done=p.done, reset=p.reset_mask, ep_stats=p.ep_stats, rewards=self.rewards,
                   dones=self.dones, deltas=self.deltas, val_prev=self.val_prev, states=self.states, bookmark=self.bookmark)
        if frames:
            out["frames"] = p.frames
        if self.h is not None:
            out.update(h=self.h, done_eff=self.done_eff)
        return out


def _compare_kernel(wname, B, C, recurrent=False, frames=True):
    from a2c_amd import ops
    _, n_act, pong, _ = WORLDS[wname]
    a, b = _Side(wname, B, C, recurrent), _Side(wname, B, C, recurrent)      # a: the launch sequence, b: one launch
    acts = torch.from_numpy(action_stream(wname, B)).to(DEV)
    g = torch.Generator().manual_seed(B * 10 + C)
    vals = torch.randn((N_STEPS, B, 2), generator=g).to(DEV)                # val_stride = 2
    hs = torch.randn((N_STEPS, B, 5), generator=g).to(DEV)
    seen = dict(reset=0, done_only=0, rew_only=0)
    HW, S = a.HW, a.S
    for k in range(N_STEPS):
        t = k % T
        if t == 0:       # state 0 of a slot = the bookmark
            for x in (a, b):
                x.states.view(-1, T, S)[x.slot0:, 0] = x.bookmark
        if recurrent:
            a.h.copy_(hs[k]); b.h.copy_(hs[k])
        ap, v = (acts[k].data_ptr(), 1), vals[k]
        # a: step, then the bookkeeping and the frame stack the eager rollout issues for this kind of net
        fr, rew, done, reset = a.pool.device_step(t, 0, B, actions=ap)
        nxt, nstride = a.rows(t)
        if recurrent:
            ops.rollout_record(rew, done, v.data_ptr(), 2, a.val_prev, a.rewards, a.dones, a.deltas, a.done_eff, a.h, B, T, t,
                               a.slot0, GAMMA, pong)
            ops.frame_stack_push(fr, reset, a.sp(t), T * S, nxt, nstride, B, C, HW)
        else:
            ops.rollout_post(rew, done, v.data_ptr(), 2, a.val_prev, a.rewards, a.dones, a.deltas, T, t, a.slot0, GAMMA, pong, fr,
                             reset, a.sp(t), T * S, nxt, nstride, B, C, HW)
        # b: one launch
        nxt, nstride = b.rows(t)
        post = ops.world_post(v.data_ptr(), 2, b.val_prev, b.rewards, b.dones, b.deltas, T, t, b.slot0, GAMMA, pong, b.sp(t), T * S,
                              nxt, nstride, C, done_eff=b.done_eff if recurrent else None, h=b.h)
        b.pool.device_step_post(t, 0, B, ap, post, frames=frames)
        ta, tb = a.tensors(frames), b.tensors(frames)
        for name in ta:
            assert torch.equal(ta[name], tb[name]), (wname, B, C, k, name)
        seen["reset"] += int(reset.sum())
        seen["done_only"] += int(((done != 0) & (reset == 0)).sum())
        seen["rew_only"] += int(((rew != 0) & (reset == 0)).sum())
    if not frames:       # the pool's frame rows were left alone
        assert torch.equal(b.pool.frames, _pool(wname, B).frames)
    return seen, a


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("B", [1, 7, 70])
@pytest.mark.parametrize("wname", list(WORLDS))
def test_one_launch_equals_step_then_rollout_post(wname, B, C):
    assert_the_action_stream_shows_every_event(wname)
    seen, a = _compare_kernel(wname, B, C)
    print(f"{wname} B={B} C={C}: {seen}, episodes {a.pool.ep_stats.tolist()}")
    if B == 7:      # the worlds of the twins: the same events happened on the device
        resets, done_only, rew_only = twin_events(wname, WORLDS[wname][3])
        assert seen["reset"] == int(resets.sum()) and seen["rew_only"] == rew_only and seen["done_only"] == done_only
        assert seen["reset"] >= B and seen["rew_only"] >= 1 and (wname != "pong" or seen["done_only"] >= 1)
    assert float(a.deltas[a.slot0 * T:].abs().max()) > 0


@pytest.mark.parametrize("wname", list(WORLDS))
def test_frames_may_be_null(wname):
    _compare_kernel(wname, 7, 3, frames=False)


@pytest.mark.parametrize("B", [7, 70])
@pytest.mark.parametrize("wname", list(WORLDS))
def test_recurrent_form_equals_step_record_push(wname, B):
    seen, a = _compare_kernel(wname, B, 3, recurrent=True)
    assert seen["reset"] >= 1 and float(a.h.abs().max()) > 0


# ---------------------------------------------------------------- argument checks
def _err_arg_cases(wname):
    """-> (call(**overrides) -> return code, buffers): a valid B = 2 call of a2c_<world>_step_post; every output is a buffer
    filled with a canary value, so that a launch that slipped through a check would show anywhere in or around it"""
    from a2c_amd import _lib
    lib = _lib.load()
    B, C = 2, 2
    pool = _pool(wname, B)
    HW = pool.HW
    f32 = dict(dtype=torch.float32, device=DEV)
    bufs = {n: torch.full((4 * C * HW + 64,), -3.0, **f32) for n in ("out", "prev", "frames")}
    bufs.update({n: torch.full((64,), -3.0, **f32) for n in ("rew", "done", "reset", "val", "val_prev", "rewards", "dones",
                                                              "deltas", "done_eff", "h")})
    bufs["stats"] = torch.full((64,), -3, dtype=torch.int32, device=DEV)
    acts = torch.zeros(B, dtype=torch.int64, device=DEV)
    ptr = {n: x.data_ptr() + 64 for n, x in bufs.items()}      # 16 floats of canary in front of every output

    def call(**o):
        a = dict(state=pool.state.data_ptr(), actions=acts.data_ptr(), stride=1, B=B, env0=0, frames=ptr["frames"], ld=HW,
                 rew=ptr["rew"], done=ptr["done"], reset=ptr["reset"], post=True, val=ptr["val"], val_prev=ptr["val_prev"],
                 rewards=ptr["rewards"], dones=ptr["dones"], deltas=ptr["deltas"], T=3, t=1, C=C, prev=ptr["prev"],
                 prev_stride=C * HW, out=ptr["out"], out_stride=C * HW, h=None, hdim=0, world={})
        a.update(o)
        post = _lib.WorldPost(val=a["val"], val_stride=1, val_prev=a["val_prev"], rewards=a["rewards"], dones=a["dones"],
                              deltas=a["deltas"], T=a["T"], t=a["t"], slot0=0, gamma=GAMMA, pong=0, prev=a["prev"],
                              prev_stride=a["prev_stride"], out=a["out"], out_stride=a["out_stride"], C=a["C"],
                              done_eff_out=ptr["done_eff"], h=a["h"], hdim=a["hdim"])
        pp = ctypes.byref(post) if a["post"] else None
        head = (a["state"], a["actions"], a["stride"], 0, a["B"], a["env0"], 1)
        tail = (a["rew"], a["done"], a["reset"])
        if wname == "pong":
            w = dict(dict(points=2, steps=40, num=3, den=4), **a["world"])
            return lib.a2c_pong_step_post(*head, w["points"], w["steps"], w["num"], w["den"], a["frames"], a["ld"], *tail,
                                          ptr["stats"], ptr["stats"] + 4, pp, None)
        if wname == "breakout":
            w = dict(dict(lives=1, steps=40), **a["world"])
            return lib.a2c_breakout_step_post(*head, w["lives"], w["steps"], a["frames"], a["ld"], *tail, ptr["stats"],
                                              ptr["stats"] + 4, pp, None)
        w = dict(dict(G=5, unit=4, foods=2), **a["world"])
        return lib.a2c_snake_step_post(*head, w["G"], w["unit"], w["foods"], *tail, a["frames"], None, ptr["stats"], pp, None)
    return call, pool, bufs, ptr, HW, C


@pytest.mark.parametrize("wname", list(WORLDS))
def test_argument_checks_return_err_arg_without_launching(wname):
    call, pool, bufs, ptr, HW, C = _err_arg_cases(wname)
    state0 = pool.state.clone()
    E = -1
    bad = [dict(post=False), dict(T=0), dict(t=-1), dict(t=3), dict(C=0), dict(prev_stride=C * HW + 2), dict(out_stride=C * HW + 2),
           dict(prev_stride=C * HW - 4), dict(out_stride=C * HW - 4), dict(out=ptr["out"] + 4), dict(prev=ptr["prev"] + 8),
           dict(prev=ptr["out"]), dict(h=ptr["h"], hdim=0), dict(h=ptr["h"], hdim=-2)]
    bad += [{n: None} for n in ("val", "val_prev", "rewards", "dones", "deltas", "prev", "out")]
    # everything the world's own step rejects
    bad += [dict(state=None), dict(actions=None), dict(rew=None), dict(done=None), dict(reset=None), dict(stride=-1),
            dict(env0=-1), dict(B=-1)]
    if wname == "snake":
        bad += [dict(world=dict(G=3)), dict(world=dict(G=33)), dict(world=dict(unit=0)), dict(world=dict(unit=17)),
                dict(world=dict(foods=0)), dict(world=dict(foods=22))]
    else:
        bad += [dict(B=0), dict(frames=ptr["frames"] + 4), dict(ld=HW - 4), dict(ld=HW + 2), dict(world=dict(steps=0)),
                dict(world=dict(steps=(1 << 24) + 1))]
        bad += [dict(world=dict(points=0)), dict(world=dict(points=22)), dict(world=dict(den=0)), dict(world=dict(num=5)),
                dict(world=dict(num=-1))] if wname == "pong" else [dict(world=dict(lives=0)), dict(world=dict(lives=6))]
    for o in bad:
        assert call(**o) == E, (wname, o)
    torch.cuda.synchronize()
    assert torch.equal(pool.state, state0)
    for n, x in bufs.items():
        assert bool((x == -3).all()), (wname, n)      # nothing ran
    assert call() == 0 and call(frames=None) == 0      # ... and the valid call, with and without `frames`, is accepted
    torch.cuda.synchronize()
    assert not torch.equal(pool.state, state0)
    assert bool((bufs["out"][:16] == -3).all()) and bool((bufs["out"][16 + 2 * C * HW:] == -3).all())


# ---------------------------------------------------------------- the Runner's one-graph slot
RUNNER_B, RUNNER_T, RUNNER_ROUNDS = 4, 6, 5
# model, env_type, state shape, pool: worlds small enough that resets fall inside the 30 steps
RUNNER_CASES = {
    "fc_pong": ("FCModel", "Pong-device", (4, 80, 80), "pong", dict(points_to_win=1, max_episode_steps=25), 3),
    "grufc_pong": ("GRUFCModel", "Pong-device", (4, 80, 80), "pong", dict(points_to_win=1, max_episode_steps=25), 3),
    "a3c_breakout": ("A3CModel", "Breakout-device", (4, 80, 72), "breakout", dict(lives=1, max_episode_steps=25), 4),
    "a3c_snake": ("A3CModel", "Snake-device", (4, 84, 84), "snake", dict(grid_size=21, unit_size=4, n_foods=2), 4),
}


def _datas(N, ss, net):
    D = dict(states=torch.zeros(N, *ss, device=DEV), deltas=torch.zeros(N, device=DEV),
             rewards=torch.zeros(N, device=DEV), dones=torch.zeros(N, device=DEV),
             actions=torch.zeros(N, dtype=torch.int64, device=DEV))
    if net.is_recurrent:
        D["h_states"] = torch.zeros(N, net.h_size, device=DEV)
    return D


def _runner(case, graphs, uniform_fn, rew_q=None, seed=12, world_kw=None, **hyp):
    import a2c_amd
    from a2c_amd.breakout import DeviceBreakoutPool
    from a2c_amd.pong import DevicePongPool
    from a2c_amd.runner import Runner
    from a2c_amd.snake import DeviceSnakePool
    kind, env_type, ss, wname, world, n_act = RUNNER_CASES[case]
    world = dict(world, **(world_kw or {}))
    B, T_ = RUNNER_B, RUNNER_T
    hyps = base_hyps(env_type=env_type, n_tsteps=T_, n_rollouts=B, n_envs=B, rollout_graphs=graphs, **hyp)
    torch.manual_seed(5)
    net = getattr(a2c_amd.models, kind)(list(ss), n_act, h_size=64 if "FC" in kind else 256, bnorm=False)
    D = _datas(B * T_, ss, net)
    pool = dict(pong=DevicePongPool, breakout=DeviceBreakoutPool, snake=DeviceSnakePool)[wname](B, DEV, seed=seed, **world)
    return net, D, pool, hyps, Runner(D, hyps, None, None, rew_q, env_pool=pool, uniform_fn=uniform_fn)


def _uniforms(seed, n):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, RUNNER_T, RUNNER_B), generator=g).to(DEV)


def _play(case, graphs, update=False):
    """RUNNER_ROUNDS rollouts (eager, captured, replayed x 3 on the graph path) -> the rows after every rollout, the pool's
    state words and episode counters, the net's parameters"""
    us, rnd = _uniforms(3, RUNNER_ROUNDS), [0]
    net, D, pool, hyps, r = _runner(case, graphs, lambda t, Bn, env0: us[rnd[0], t, env0:env0 + Bn].contiguous())
    upd = None
    if update:
        from a2c_amd.updater import Updater
        upd = Updater(net, hyps)
    rows = []
    for rnd[0] in range(RUNNER_ROUNDS):
        r.rollout(net, list(range(RUNNER_B)), hyps)
        r.finish()
        rows.append({k: v.clone() for k, v in D.items()})
        if upd is not None:
            upd.update_model(D)
    torch.cuda.synchronize()
    graphs_made = [g for g in getattr(r, "_dev_graphs", {}).values()]
    return rows, (pool.state.clone(), pool.ep_stats.clone()), [p.detach().clone() for p in net.parameters()], graphs_made


@pytest.mark.parametrize("case", list(RUNNER_CASES))
def test_graph_slot_equals_the_eager_rollout(case):
    got, state, _, made = _play(case, True)
    want, state_w, _, made_w = _play(case, False)
    assert len(made) == 1 and isinstance(made[0], torch.cuda.CUDAGraph) and not made_w      # captured; and not on the comparator
    assert int(state_w[1][0]) >= RUNNER_B, "episodes end inside the rollouts"
    for k in range(RUNNER_ROUNDS):
        for name in want[k]:
            assert torch.equal(got[k][name], want[k][name]), (case, k, name)
    assert torch.equal(state[0], state_w[0]) and torch.equal(state[1], state_w[1])
    assert not torch.equal(want[3]["states"], want[4]["states"])


def test_graph_slot_with_updates_in_between():
    """the weights change after every rollout: the refresh of the kernels' weight copies, outside the graph, takes effect"""
    got, state, params, made = _play("fc_pong", True, update=True)
    want, state_w, params_w, _ = _play("fc_pong", False, update=True)
    assert isinstance(made[0], torch.cuda.CUDAGraph)
    for k in range(RUNNER_ROUNDS):
        for name in want[k]:
            assert torch.equal(got[k][name], want[k][name]), (k, name)
    assert torch.equal(state[0], state_w[0]) and torch.equal(state[1], state_w[1])
    for p, q in zip(params, params_w):
        assert torch.equal(p, q)
    plain, _, params0, _ = _play("fc_pong", False)
    assert not torch.equal(params_w[0], params0[0]) and not torch.equal(want[4]["deltas"], plain[4]["deltas"])


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


@pytest.mark.parametrize("case", ["fc_pong", "a3c_snake"])
def test_a_replayed_rollout_issues_no_launch(case):
    """no uniform_fn (the slot's uniforms are one torch.rand), no update: a rollout after the capture is the replay and
    nothing else.  The eager runner draws its uniforms step by step -- another random stream --, so the comparator is handed
    the uniforms the graph runner drew: rows, finish() and rew_q are then the same"""
    from a2c_amd import ops
    out, drawn, rnd = {}, [], [0]
    for graphs in (True, False):
        torch.manual_seed(77)
        rq = queue.Queue(1)
        rq.put(0.0)
        fn = None if graphs else (lambda t, Bn, env0: drawn[rnd[0]][t, env0:env0 + Bn].contiguous())
        # (Pong: a step limit of 10, so that episodes end inside the 24 steps whatever the policy does)
        net, D, pool, hyps, r = _runner(case, graphs, fn, rew_q=rq, world_kw=dict(max_episode_steps=10) if "pong" in case else None)
        n, rows, eps, stats = [], [], [], pool.episode_stats
        pool.episode_stats = lambda: eps.append(stats()) or eps[-1]      # what finish() read, once per rollout
        for rnd[0] in range(4):
            real, counted = ops.lib, _CountedLib(ops.lib())
            ops.lib = lambda: counted
            try:
                r.rollout(net, list(range(RUNNER_B)), hyps)
            finally:
                ops.lib = real
            r.finish()
            n.append(counted.n)
            rows.append({k: v.clone() for k, v in D.items()})
            if graphs:
                drawn.append(r._u_buf.clone())
        out[graphs] = (rows, rq.get(), n, eps)
    print(f"{case}: launches issued per rollout, graph path {out[True][2]}, eager {out[False][2]}")
    assert out[True][2][0] > 0 and out[True][2][1] > 0 and out[True][2][2:] == [0, 0]
    assert min(out[False][2]) > 0
    assert not torch.equal(drawn[2], drawn[3])
    for k in range(4):
        for name in out[False][0][k]:
            assert torch.equal(out[True][0][k][name], out[False][0][k][name]), (k, name)
    assert out[True][1] == out[False][1] and out[True][3] == out[False][3]
    assert len(out[True][3]) == 4 and sum(k for k, _ in out[True][3]) >= RUNNER_B      # one read per rollout; episodes ended


def test_under_an_outer_capture():
    """a rollout captured by the caller and replayed twice == two rollouts of an untouched runner; the captured runner
    starts no capture of its own there, and afterwards still captures and replays its own graph"""
    from a2c_amd import ops
    us = _uniforms(8, 1)[0]
    fn = lambda t, Bn, env0: us[t, env0:env0 + Bn]
    idx = list(range(RUNNER_B))

    def make():
        net, D, pool, hyps, r = _runner("fc_pong", True, fn, seed=2)
        r.rollout(net, idx, hyps)                  # warm rollout
        torch.cuda.synchronize()
        return net, D, pool, hyps, r
    net, D, pool, hyps, r = make()
    want = []
    for _ in range(4):
        r.rollout(net, idx, hyps)
        torch.cuda.synchronize()
        want.append({k: v.clone() for k, v in D.items()})
    state_w = pool.state.clone()
    net, D, pool, hyps, r = make()
    g = torch.cuda.CUDAGraph()
    state0 = pool.state.clone()
    with ops.graph_capture(g):
        r.rollout(net, idx, hyps)
    torch.cuda.synchronize()
    assert torch.equal(pool.state, state0), "capturing plays nothing"
    assert list(r._dev_graphs.values()) == ["warm"]            # its own state was left alone
    for k in range(2):
        g.replay()
        torch.cuda.synchronize()
        for name in D:
            assert torch.equal(D[name], want[k][name]), (k, name)
    for k in (2, 3):                                            # its own capture, then its own replay
        r.rollout(net, idx, hyps)
        torch.cuda.synchronize()
        for name in D:
            assert torch.equal(D[name], want[k][name]), (k, name)
    assert isinstance(list(r._dev_graphs.values())[0], torch.cuda.CUDAGraph)
    assert torch.equal(pool.state, state_w)


def test_train_graph_path_equals_rollout_graphs_false(tmp_path):
    from a2c_amd.training import train
    us = _uniforms(21, 1)[0]
    params = {}
    for graphs in (True, False):
        hyps = dict(exp_name=f"pong_{int(graphs)}", main_path=str(tmp_path), model="FCModel", env_type="Pong-device",
                    n_envs=RUNNER_B, n_rollouts=RUNNER_B, n_tsteps=RUNNER_T, n_frame_stack=3, max_tsteps=1e9, seed=1,
                    points_to_win=1, max_episode_steps=10, h_size=32, n_test_eps=2, max_eval_steps=5)
        if not graphs:
            hyps["rollout_graphs"] = False
        torch.manual_seed(3)
        train(None, hyps, verbose=False, max_epochs=3, uniform_fn=lambda t, Bn, env0: us[t, env0:env0 + Bn],
              on_epoch=lambda epoch, upd, D: params.setdefault(graphs, []).append(
                  [p.detach().clone() for p in upd.net.parameters()]))
    assert len(params[True]) == 3 and len(params[False]) == 3
    for p, q in zip(params[True][-1], params[False][-1]):
        assert torch.equal(p, q)
    assert not torch.equal(params[True][0][0], params[True][-1][0])
