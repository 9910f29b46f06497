"""-m gpu: the CartPole worlds in device memory (csrc/cartpole.hip, a2c_amd.cartpole.DeviceCartPolePool) against the host twin
``CartPoleEnv`` after every step; the post form against its launch sequence; the Runner with the discrete FC nets on the
device pool against host twins, and its graph path against the eager loop; the ``DeviceStatsRunner`` against the host
``StatsRunner``; ``train()``; the custom-op binding.  The world is integers and the observations are exact fractions, so every
comparison is ``torch.equal``."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import base_hyps  # noqa: E402
from test_cartpole import RULES, host_play  # noqa: E402

DEV = "cuda"
GAMMA = 0.99
N_STEPS, ENV_ID0 = 600, 7
CAUSES = ("x_limit", "theta_limit", "step_limit")


def dev(a):
    """a (read-only) host array as a device tensor"""
    return torch.from_numpy(np.array(a)).to(DEV)


def _pool(B, rules="plain", seed=5, cap=60, env_id0=ENV_ID0, **kw):
    from a2c_amd.cartpole import DeviceCartPolePool
    return DeviceCartPolePool(B, DEV, seed=seed, max_episode_steps=cap, env_id0=env_id0, **RULES[rules], **kw)


# ---------------------------------------------------------------- 1. device against twins, after every step
@pytest.mark.parametrize("cap", [60, 500])
@pytest.mark.parametrize("B,rules,shift", [(1, "plain", 0), (64, "plain", 0), (65, "plain", 0), (130, "plain", 0), (65, "repeat", 3)])
def test_device_worlds_equal_the_host_twins(B, rules, shift, cap):
    """env ids 7 .., 600 agent steps; even ids hashed actions, odd ids the controller of test_cartpole.py.  The worlds of
    max_episode_steps = 60 end by theta_limit and step_limit; no cart can leave the track inside 60 frames with the pole up
    (test_cartpole.py says why), so the SAME streams are also played on worlds of 500, which end by x_limit: between the two,
    every cause is compared on the device -- the precondition is checked on the twins first.  The repeat case reads its actions
    from env-major rows with action_shift = 3"""
    n = N_STEPS
    h = host_play(B, n, rules, cap, shift)
    if B >= 64:
        ev = [host_play(B, n, rules, c, shift)["events"] for c in (60, 500)]
        assert all(ev[0][k] + ev[1][k] >= 1 for k in CAUSES) and ev[1]["x_limit"] >= 1 and ev[0]["step_limit"] >= 1, ev
        assert all(h["events"][k] >= 1 for k in (("cut", "sticky") if rules == "repeat" else ())), h["events"]
    pool = _pool(B, rules, cap=cap)
    pool.action_shift = shift
    want = {k: dev(h[k]) for k in ("rew", "done", "obs")}
    want["words"], want["stats"] = dev(h["words"].astype(np.int32)), dev(h["stats"].astype(np.int32))
    if rules == "repeat":      # env-major rows like a rollout buffer's: stride n, step t at an offset of t elements
        acts, stride, off = dev(np.ascontiguousarray(h["acts"].T)), n, 8
    else:
        acts, stride, off = dev(h["acts"]), 1, 8 * B
    pool.reset_all()
    assert torch.equal(pool.frames, want["obs"][0]), "reset observations"
    assert torch.equal(pool.state[:, :4], dev(np.round(h["obs"][0].astype(np.float64) * 2 ** 20).astype(np.int32)))
    bad = torch.zeros(6, dtype=torch.int64, device=DEV)      # mismatches: words, obs, rew, done, reset, counters
    for t in range(n):
        fr, r, d, rs = pool.step(acts.data_ptr() + off * t, stride)
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
    assert int(h["stats"][-1][0]) >= 1


def test_sub_range_stepping_equals_one_call():
    """env0 / B blocks of a 130-env pool, cut inside and at the end of a wavefront, give what one call gives"""
    B, T = 130, 40
    acts = dev(host_play(B, N_STEPS, "plain", 60)["acts"][:T])
    whole, parts = _pool(B, "repeat"), _pool(B, "repeat")
    whole.reset_all()
    parts.reset_all()
    with pytest.raises(ValueError):
        parts.step(acts[0].data_ptr(), 1, env0=100, B=31)
    for t in range(T):
        whole.step(acts[t].data_ptr(), 1)
        for env0, n in ((0, 64), (64, 1), (65, 65)):
            fr, r, d, rs = parts.device_step(t, env0, n, actions=(acts[t].data_ptr() + 8 * env0, 1))
            assert fr.shape == (n, 4) and r.shape == d.shape == rs.shape == (n,)
        for name in ("state", "frames", "rew", "done", "reset_mask", "ep_stats"):
            assert torch.equal(getattr(whole, name), getattr(parts, name)), (t, name)
    assert int(whole.ep_stats[0]) > 0


# ---------------------------------------------------------------- 2. the post form against its launch sequence
T = 3
POST_STEPS, POST_CAP = 40, 9


class _Side:
    """one pool and one set of rollout buffers, rows addressed as in the Runner's buffers: slot0 + b, T rows per slot"""

    def __init__(self, B, C, rules, hdim):
        from a2c_amd import ops
        self.pool = _pool(B, rules, cap=POST_CAP)
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
        self.h = torch.zeros((B, hdim), **f32) if hdim else None

    def sp(self, t):
        return self.states.data_ptr() + 4 * (self.slot0 * T + t) * self.S

    def rows(self, t):
        return (self.sp(t + 1), T * self.S) if t + 1 < T else (self.bookmark.data_ptr(), self.S)

    def tensors(self):
        p = self.pool
        out = dict(state=p.state, rew=p.rew, done=p.done, reset=p.reset_mask, ep_stats=p.ep_stats, rewards=self.rewards,
                   dones=self.dones, deltas=self.deltas, val_prev=self.val_prev, states=self.states, bookmark=self.bookmark,
                   done_eff=self.done_eff)
        if self.h is not None:
            out["h"] = self.h
        return out


@pytest.mark.parametrize("hdim", [0, 16, 200])
@pytest.mark.parametrize("rules", list(RULES))
@pytest.mark.parametrize("C", [1, 4])
def test_post_form_equals_its_launch_sequence(C, rules, hdim):
    """B = 65, 40 steps: one a2c_cartpole_step with a post block == the plain step, then a2c_rollout_record +
    a2c_frame_stack_push; the hidden rows of closed envs are zeroed and the others untouched"""
    from a2c_amd import ops
    B = 65
    a, b = _Side(B, C, rules, hdim), _Side(B, C, rules, hdim)      # a: the launch sequence, b: one launch
    acts = dev(host_play(B, N_STEPS, "plain", 60)["acts"][:POST_STEPS])
    g = torch.Generator().manual_seed(10 * C + hdim)
    vals = torch.randn((POST_STEPS, B, 2), generator=g).to(DEV)              # val_stride = 2
    hs = torch.randn((POST_STEPS, B, max(hdim, 1)), generator=g).to(DEV)
    S, closed = a.S, 0
    obs0 = b.pool.frames.clone()
    for k in range(POST_STEPS):
        t = k % T
        if t == 0:       # state 0 of a slot = the bookmark
            for x in (a, b):
                x.states.view(-1, T, S)[x.slot0:, 0] = x.bookmark
        if hdim:
            a.h.copy_(hs[k]); b.h.copy_(hs[k])
        ap, v = (acts[k].data_ptr(), 1), vals[k]
        fr, rew, done, reset = a.pool.device_step(t, 0, B, actions=ap)
        nxt, nstride = a.rows(t)
        ops.rollout_record(rew, done, v.data_ptr(), 2, a.val_prev, a.rewards, a.dones, a.deltas, a.done_eff, a.h, B, T, t,
                           a.slot0, GAMMA, False)
        ops.frame_stack_push(fr, reset, a.sp(t), T * S, nxt, nstride, B, C, 4)
        nxt, nstride = b.rows(t)
        post = ops.world_post(v.data_ptr(), 2, b.val_prev, b.rewards, b.dones, b.deltas, T, t, b.slot0, GAMMA, False, b.sp(t),
                              T * S, nxt, nstride, C, done_eff=b.done_eff, h=b.h)
        b.pool.device_step_post(t, 0, B, ap, post)
        ta, tb = a.tensors(), b.tensors()
        for name in ta:
            assert torch.equal(ta[name], tb[name]), (C, k, name)
        if hdim:
            rows = done.bool()
            assert bool((b.h[rows] == 0).all()) and torch.equal(b.h[~rows], hs[k][~rows])
        closed += int(reset.sum())
    print(f"cartpole post C={C} {rules} hdim={hdim}: closed {closed}, episodes {a.pool.ep_stats.tolist()}")
    assert closed >= B and float(a.deltas[a.slot0 * T:].abs().max()) > 0
    assert torch.equal(b.pool.frames, obs0), "obs == NULL: the pool's observation rows were left alone"


def test_post_form_with_observation_rows():
    from a2c_amd import ops
    B, C = 65, 4
    a, b = _Side(B, C, "repeat", 16), _Side(B, C, "repeat", 16)
    acts = dev(host_play(B, N_STEPS, "plain", 60)["acts"][:6])
    v = torch.randn((B,), generator=torch.Generator().manual_seed(1)).to(DEV)
    for k in range(6):
        a.pool.step(acts[k].data_ptr(), 1)
        post = ops.world_post(v.data_ptr(), 1, b.val_prev, b.rewards, b.dones, b.deltas, T, 0, b.slot0, GAMMA, False, b.sp(0),
                              T * b.S, b.sp(1), T * b.S, C, done_eff=b.done_eff, h=b.h)
        b.pool.device_step_post(0, 0, B, (acts[k].data_ptr(), 1), post, frames=True)
        assert torch.equal(a.pool.frames, b.pool.frames) and torch.equal(a.pool.state, b.pool.state)


def test_valid_calls_are_accepted_and_write_inside_their_rows():
    """the refusals are test_cartpole.py's (no launch); here the calls they are variations of run, and stay inside their rows"""
    import ctypes
    from a2c_amd import _lib
    lib = _lib.load()
    B, C, HW = 2, 2, 4
    pool = _pool(B)
    pool.reset_all()
    f32 = dict(dtype=torch.float32, device=DEV)
    bufs = {n: torch.full((256,), -3.0, **f32) for n in ("out", "prev", "obs", "rew", "done", "reset", "val", "val_prev",
                                                         "rewards", "dones", "deltas", "h")}
    acts = torch.zeros(B, dtype=torch.int64, device=DEV)
    ptr = {n: x.data_ptr() + 64 for n, x in bufs.items()}      # 16 floats of canary in front of every output

    def step(post=False, obs=ptr["obs"], h=None, hdim=0, rules=None):
        blk = _lib.WorldPost(val=ptr["val"], val_stride=1, val_prev=ptr["val_prev"], rewards=ptr["rewards"], dones=ptr["dones"],
                             deltas=ptr["deltas"], T=3, t=1, slot0=0, gamma=GAMMA, pong=0, prev=ptr["prev"], prev_stride=C * HW,
                             out=ptr["out"], out_stride=C * HW, C=C, done_eff_out=None, h=h, hdim=hdim)
        return lib.a2c_cartpole_step(pool.state.data_ptr(), acts.data_ptr(), 1, 0, B, 0, 1, 40, obs, HW, ptr["rew"], ptr["done"],
                                     ptr["reset"], None, None, None if rules is None else ctypes.byref(rules),
                                     ctypes.byref(blk) if post else None, None)
    state0 = pool.state.clone()
    assert step(obs=None) == -1 and step(post=True, h=ptr["h"], hdim=0) == -1
    torch.cuda.synchronize()
    assert torch.equal(pool.state, state0) and all(bool((x == -3).all()) for x in bufs.values())
    R = _lib.WorldRules
    assert step() == 0 and step(post=True) == 0 and step(post=True, obs=None) == 0 and step(rules=R(2, 4, 1, 4, 0, 0)) == 0
    assert step(post=True, h=ptr["h"], hdim=5, rules=R(1, 1, 0, 1, 0, 0)) == 0
    assert lib.a2c_cartpole_reset(pool.state.data_ptr(), B, 0, 1, 40, ptr["obs"], HW, None) == 0
    torch.cuda.synchronize()
    assert not torch.equal(pool.state, state0)
    assert bool((bufs["out"][:16] == -3).all()) and bool((bufs["out"][16 + 2 * C * HW:] == -3).all())
    assert bool((bufs["obs"][:16] == -3).all()) and bool((bufs["obs"][16 + B * HW:] == -3).all())
    assert bool((bufs["obs"][16:16 + B * HW] != -3).all())
    assert bool((bufs["h"] == -3).all())              # no env closed: no hidden row was cleared
    for n in ("rew", "done", "reset"):
        assert bool((bufs[n][16 + B:] == -3).all()) and bool((bufs[n][:16] == -3).all()), n


# ---------------------------------------------------------------- 3. / 4. through the Runner
RUNNER_CAP = 9                                                   # every world ends episodes inside the rollouts
RUNNER_B, RUNNER_T, RUNNER_ROUNDS = 5, 6, 3
KINDS = ("FCModel", "GRUFCModel")


def _net(kind, C=4, seed=5):
    import a2c_amd
    torch.manual_seed(seed)
    return getattr(a2c_amd.models, kind)([C, 4], 2, h_size=32, bnorm=False)


def _datas(N, net, C=4):
    D = dict(states=torch.zeros(N, C, 4, device=DEV), deltas=torch.zeros(N, device=DEV), rewards=torch.zeros(N, device=DEV),
             dones=torch.zeros(N, device=DEV), actions=torch.zeros(N, dtype=torch.int64, device=DEV))
    if net.is_recurrent:
        D["h_states"] = torch.zeros(N, net.h_size, device=DEV)
    return D


def _uniforms(seed, n, T_=RUNNER_T, B=RUNNER_B):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, T_, B), generator=g).to(DEV)


def _hyps(**kw):
    return base_hyps(**dict(dict(env_type="CartPole-device", n_tsteps=RUNNER_T, n_rollouts=RUNNER_B, n_envs=RUNNER_B, h_size=32),
                            **kw))


class _CountedLib:
    """the library with the calls of every launching a2c_* entry point counted by name"""

    def __init__(self, lib):
        self._lib, self.n, self.by_name = lib, 0, {}

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("a2c_") or name.endswith(("_bytes", "_supported", "_splits", "_version", "_string")):
            return f

        def counted(*a):
            self.n += 1
            self.by_name[name] = self.by_name.get(name, 0) + 1
            return f(*a)
        return counted


def _play(kind, pool_kind, graphs, rules="plain", rounds=RUNNER_ROUNDS):
    """``rounds`` rollouts of the same net with the same uniforms on a DeviceCartPolePool or on a HostEnvPool of twins -> the
    rows after every rollout, the launches every rollout issued, the graphs made, the pool"""
    from a2c_amd import ops
    from a2c_amd.cartpole import CartPoleEnv, DeviceCartPolePool
    from a2c_amd.runner import HostEnvPool, Runner
    us, rnd = _uniforms(3, rounds), [0]
    hyps = _hyps(rollout_graphs=graphs)
    net = _net(kind)
    D = _datas(RUNNER_B * RUNNER_T, net)
    if pool_kind == "device":
        pool = DeviceCartPolePool(RUNNER_B, DEV, seed=12, max_episode_steps=RUNNER_CAP, **RULES[rules])
    else:
        pool = HostEnvPool([CartPoleEnv(seed=12, env_id=j, max_episode_steps=RUNNER_CAP, **RULES[rules]) for j in range(RUNNER_B)],
                           frame_shape=(1, 4))
    r = Runner(D, hyps, None, None, None, env_pool=pool, uniform_fn=lambda t, Bn, env0: us[rnd[0], t, env0:env0 + Bn].contiguous())
    rows, launches = [], []
    for rnd[0] in range(rounds):
        real, counted = ops.lib, _CountedLib(ops.lib())
        ops.lib = lambda: counted
        try:
            r.rollout(net, list(range(RUNNER_B)), hyps)
        finally:
            ops.lib = real
        r.finish()
        launches.append(counted.n)
        rows.append({k: v.clone() for k, v in D.items()})
    torch.cuda.synchronize()
    return rows, launches, list(getattr(r, "_dev_graphs", {}).values()), pool


@pytest.mark.parametrize("kind", KINDS)
def test_slot_graph_equals_the_eager_loop(kind):
    got, n, made, pool = _play(kind, "device", True)
    want, n_w, made_w, pool_w = _play(kind, "device", False)
    print(f"cartpole {kind}: launches per rollout, graph path {n}, eager {n_w}")
    assert len(made) == 1 and isinstance(made[0], torch.cuda.CUDAGraph) and not made_w      # captured; not on the comparator
    assert n[0] > 0 and n[1] > 0 and n[2] == 0 and min(n_w) > 0, "the third rollout is the replay and nothing else"
    assert int(pool_w.ep_stats[0]) >= RUNNER_B, "episodes end inside the rollouts"
    for k in range(RUNNER_ROUNDS):
        for name in want[k]:
            assert torch.equal(got[k][name], want[k][name]), (kind, k, name)
    assert torch.equal(pool.state, pool_w.state) and torch.equal(pool.ep_stats, pool_w.ep_stats)
    assert int(pool.state[0, 5]) >= RUNNER_ROUNDS * RUNNER_T, "the replay played new steps"
    assert not torch.equal(want[1]["states"], want[2]["states"])


@pytest.mark.parametrize("rules", list(RULES))
@pytest.mark.parametrize("kind", KINDS)
def test_runner_device_pool_equals_host_twins(kind, rules):
    d, _, _, pool = _play(kind, "device", False, rules)
    h, _, _, twins = _play(kind, "host", False, rules)
    ends = sum(e.events["episode_end"] for e in twins.envs)
    print(f"cartpole runner {kind} {rules}: host twins episode ends {ends}")
    assert ends >= RUNNER_B
    for k in range(RUNNER_ROUNDS):
        for name in h[k]:
            assert torch.equal(d[k][name], h[k][name]), (k, name)
    assert set(h[0]["actions"].unique().tolist()) == {0, 1} and float(h[0]["dones"].sum()) >= 1


# ---------------------------------------------------------------- 5. evaluation on the device
@pytest.mark.parametrize("kind", KINDS)
def test_device_stats_runner_equals_the_host_stats_runner(kind):
    """the same worlds (env ids 10007 ..) and uniforms: 5 episodes on the device against StatsRunner's lock-step loop over host
    twins.  max_episode_steps = 40 ends every episode, whatever the net does, before max_eval_steps = 64"""
    from a2c_amd.cartpole import CartPoleEnv, DeviceCartPolePool
    from a2c_amd.runner import DeviceStatsRunner, StatsRunner
    E, K, cap = 5, 8, 64
    hyps = _hyps(n_test_eps=E, eval_chunk=K, max_eval_steps=cap)
    us = torch.rand((2 * cap, E), generator=torch.Generator().manual_seed(9)).to(DEV)
    fn = lambda t, En, env0=0: us[t, env0:env0 + En].contiguous()
    net = _net(kind)
    dsr = DeviceStatsRunner(hyps, DeviceCartPolePool(E, DEV, seed=4, max_episode_steps=40), uniform_fn=fn, keep_actions=True)
    for call in range(2):      # the second call plays the next E worlds
        twins = [CartPoleEnv(seed=4, env_id=10007 + call * E + j, max_episode_steps=40) for j in range(E)]
        got = dsr.rollout(net)
        want = StatsRunner(hyps, envs=twins, uniform_fn=fn).rollout(net)
        last = dsr.last
        print(f"cartpole eval {kind} call {call}: {got} ep_len {last['ep_len'].tolist()} steps {last['steps']}")
        assert got == want and got > 0
        assert int(last["active"].sum()) == 0 and 1 <= int(last["ep_len"].max()) <= 40
        assert float(last["ep_rew"].sum()) == float(last["ep_len"].sum()) == got * E, "the reward is 1 a frame"
        assert sum(e.events["episode_end"] for e in twins) == E


# ---------------------------------------------------------------- 6. train()
@pytest.mark.parametrize("eval_pool", ["host", "device"])
@pytest.mark.parametrize("model,bptt", [("FCModel", False), ("GRUFCModel", True)])
def test_train_two_epochs_and_the_checkpoint_reloads(model, bptt, eval_pool, tmp_path):
    import a2c_amd
    from a2c_amd.training import train
    hyps = dict(exp_name="cartpole", main_path=str(tmp_path), model=model, env_type="CartPole-device", n_envs=8, n_rollouts=8,
                n_tsteps=8, n_frame_stack=3, max_tsteps=1e9, seed=1, max_episode_steps=30, h_size=32, n_test_eps=3,
                max_eval_steps=64, use_bptt=bptt, eval_pool=eval_pool, frame_skip=1, frame_skip_max=2)
    seen, kept = [], {}

    def on_epoch(epoch, upd, D):
        seen.append((tuple(D["states"].shape), tuple(D["actions"].shape), D["actions"].dtype, float(D["dones"].sum()),
                     float(D["rewards"].min()), dict(upd.info)))
        kept.update(net=upd.net, states=D["states"].clone())
    best = train(None, hyps, verbose=False, max_epochs=2, on_epoch=on_epoch)
    assert len(seen) == 2 and seen[0][0] == (64, 3, 4) and seen[0][1] == (64,) and seen[0][2] == torch.int64
    assert seen[0][3] + seen[1][3] >= 1 and seen[0][4] >= 1.0 and np.isfinite(best) and best > 0
    folder = os.path.join(str(tmp_path), "cartpole", "cartpole_0")
    log = open(os.path.join(folder, "log.txt")).read()
    assert "BestRew:" in log and "env_type:CartPole-device" in log
    for row in seen:
        assert row[5] and all(np.isfinite(float(v)) for v in row[5].values()), row[5]
    # net.p reloads into a fresh net and reproduces the forward bit for bit
    net = kept["net"]
    fresh = getattr(a2c_amd.models, model)([3, 4], 2, h_size=32, bnorm=False)
    fresh.load_state_dict(torch.load(os.path.join(folder, "net.p")))
    fresh = fresh.cuda()
    x = kept["states"][:8]
    with torch.no_grad():
        if net.is_recurrent:
            h0 = torch.zeros(8, net.h_size, device=DEV)
            a, b = net(x, h0), fresh(x, h0.clone())
        else:
            a, b = net(x), fresh(x)
    for p, q in zip(a, b):
        assert torch.equal(p, q) and bool(torch.isfinite(p).all())


@pytest.mark.parametrize("env_pool", ["serial", "process"])
def test_train_plays_the_host_twins_behind_the_env_pools(env_pool, tmp_path):
    from a2c_amd.training import train
    hyps = dict(exp_name="cartpole", main_path=str(tmp_path), model="FCModel", env_type="CartPole-host", n_envs=4, n_rollouts=4,
                n_tsteps=6, n_frame_stack=2, max_tsteps=1e9, seed=1, max_episode_steps=12, h_size=32, n_test_eps=2,
                max_eval_steps=32, env_pool=env_pool, n_env_workers=2)
    seen = []
    best = train(None, hyps, verbose=False, max_epochs=2,
                 on_epoch=lambda epoch, upd, D: seen.append((tuple(D["states"].shape), float(D["dones"].sum()),
                                                             float(D["states"].abs().max()))))
    assert len(seen) == 2 and seen[0][0] == (24, 2, 4) and seen[0][1] + seen[1][1] >= 1 and 0 < seen[0][2] < 8
    assert np.isfinite(best) and best > 0


# ---------------------------------------------------------------- 7. the custom-op binding
def test_rollout_through_torch_custom_ops_is_bit_identical(monkeypatch):
    """A2C_TORCH_OPS=1: the launches whose pointers live in torch tensors go through torch.ops.a2c_mi355x.abi_* (the reset among
    them); a2c_cartpole_step takes argument blocks and stays a ctypes call, like a2c_point_step -- it is counted all the same"""
    from a2c_amd import ops
    want, n_w, _, pool_w = _play("GRUFCModel", "device", False, "repeat")
    monkeypatch.setenv("A2C_TORCH_OPS", "1")
    ab = ops.torch_abi()
    ab.stats.update(torch_ops=0, ctypes=0, by_name={}, unresolved={})
    steps = []
    real = ab._c.a2c_cartpole_step
    monkeypatch.setitem(ab._fns, "a2c_cartpole_step", lambda *a: steps.append(1) or real(*a))
    got, n, _, pool = _play("GRUFCModel", "device", False, "repeat")
    monkeypatch.delenv("A2C_TORCH_OPS")
    print(f"cartpole through torch ops: {ab.stats['torch_ops']} abi_* launches, a2c_cartpole_step x {len(steps)}, "
          f"unresolved {ab.stats['unresolved']}")
    assert len(steps) == RUNNER_ROUNDS * RUNNER_T and ab.stats["by_name"].get("a2c_cartpole_reset", 0) == 1
    assert ab.stats["torch_ops"] > 20 and "a2c_cartpole_reset" not in ab.stats["unresolved"]
    for k in range(RUNNER_ROUNDS):
        for name in want[k]:
            assert torch.equal(got[k][name], want[k][name]), (k, name)
    assert torch.equal(pool.state, pool_w.state)
