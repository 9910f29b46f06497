"""-m gpu: random frame skip, episodic life and reward clipping on the device Pong and Breakout worlds
(a2c_<world>_step_rules) against the host twins -- value for value after every agent step, on the
plays tests/test_world_rules.py has shown to exercise every new rule on the twins alone --, a default rules block against
today's entry points, the one-launch form against the launch sequence it replaces, the new argument checks, and through
the Runner, the DeviceStatsRunner and ``train()``.  The worlds produce integers and frames of a few grey levels: every
comparison is exact but for the rollout's rewards and deltas against the host pool (they hold the nets' values: 1e-5,
as in test_gpu_world_skip.py)."""
import ctypes
import os
import queue

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import base_hyps  # noqa: E402
from test_gpu_kernels import close  # noqa: E402
from test_gpu_world_skip import NATURAL, _Prepped, _classes, _i32  # noqa: E402
from test_world_rules import (PLANT_ROWS, assert_every_rule_is_seen, cfg_id, play_cases, rule_kw, rules_play)  # noqa: E402
from test_world_skip import N_ACT, action_tape  # noqa: E402

DEV = "cuda"
GAMMA = 0.99
PREV_WORD = {"pong": 12, "breakout": 17}
PLANTED = sum(bin(m).count("1") for m in PLANT_ROWS)


# ---------------------------------------------------------------- 1. the device worlds equal the twins
@pytest.mark.parametrize("world,B,cfg", play_cases(), ids=lambda v: cfg_id(v) if isinstance(v, tuple) else str(v))
def test_device_worlds_equal_the_host_twins_after_every_agent_step(world, B, cfg):
    h = rules_play(world, B, cfg)
    n = h["n"]
    print(f"rules parity {world} B={B} cfg={cfg}: host twin events {h['events']}")
    assert_every_rule_is_seen(world, cfg, h)                                    # on the host twins alone
    pool = _classes(world)[0](B, DEV, seed=h["seed"], **rule_kw(world, cfg), **h["world"])
    assert pool.rules is not None and not pool.plain
    pool.reset_all()
    if world == "breakout":      # the planted wall: the position goes in through the state words
        pool.state.copy_(_i32(h["words"][0]))
    else:
        assert torch.equal(pool.frames, torch.from_numpy(np.array(h["frames"][0])).to(DEV).float()), "reset frames"
        assert np.array_equal(pool.state.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, h["words"][0]), "reset state"
    d_acts = torch.from_numpy(np.array(h["acts"])).to(DEV)
    want = {k: torch.from_numpy(np.array(h[k])).to(DEV) for k in ("rew", "done", "reset", "words")}
    frames = torch.from_numpy(np.array(h["frames"])).to(DEV)
    bad = torch.zeros(5, dtype=torch.int64, device=DEV)       # mismatches: rew, done, reset, frames, state words
    stats = []
    for t in range(n):
        fr, r, d, rs = pool.step(d_acts[t].data_ptr(), 1)
        bad[0] += (r != want["rew"][t]).sum()
        bad[1] += (d != want["done"][t]).sum()
        bad[2] += (rs != want["reset"][t]).sum()
        bad[3] += (fr != frames[t + 1].float()).sum()
        bad[4] += ((pool.state.long() & 0xFFFFFFFF) != want["words"][t + 1]).sum()
        stats.append(pool.ep_stats.clone())
    torch.cuda.synchronize()
    assert bad.tolist() == [0, 0, 0, 0, 0], bad.tolist()
    assert np.array_equal(torch.stack(stats).cpu().numpy(), h["closed"]), "episode counters after every agent step"
    if cfg[2] == 0:
        assert (pool.state[:, PREV_WORD[world]] == 0).all()
    assert pool.episode_stats() == (int(h["closed"][-1, 0]), int(h["closed"][-1, 1]))


# ---------------------------------------------------------------- 2. a default rules block is the old entry point
def _step_rules(world, pool, acts_ptr, rules, post=None, frames=True):
    """a2c_<world>_step_rules on the pool's own buffers, whatever the pool itself would call"""
    from a2c_amd import ops
    fn = ops.pong_step_rules if world == "pong" else ops.breakout_step_rules
    fn(pool.state, acts_ptr, 1, pool.action_shift, pool.B, pool.env_id0, pool.seed, *pool.world, pool.frames if frames else None,
       pool.HW, pool.rew, pool.done, pool.reset_mask, rules, post, pool.ep_stats[0:1], pool.ep_stats[1:2])


@pytest.mark.parametrize("repeat", [(1, 0, 1), (4, 1, 4)], ids=["step", "step_skip"])
@pytest.mark.parametrize("world", ["pong", "breakout"])
def test_default_rules_block_equals_todays_entry_points(world, repeat):
    """frame_skip_max == frame_skip, both flags 0: bit for bit a2c_<world>_step / _step_post (repeat (1, 0, 1)) and
    a2c_<world>_step_skip / _step_post_skip, with and without ``post``"""
    from a2c_amd import ops
    B, n, C, T = 7, 60, 2, 3
    kw = dict(zip(("frame_skip", "sticky_num", "sticky_den"), repeat))
    rules = ops.world_rules(*repeat, always=True)
    assert (rules.frame_skip_max, rules.episodic_life, rules.clip_rewards) == (repeat[0], 0, 0)
    acts = torch.from_numpy(action_tape(world, 1, B, n)).to(DEV)
    old, new, old_p, new_p = (_classes(world)[0](B, DEV, seed=3, **kw, **NATURAL[world]) for _ in range(4))
    for p in (old, new, old_p, new_p):
        assert p.rules is None and p.plain == (repeat == (1, 0, 1))
        p.reset_all()
    HW = old.HW
    f32 = dict(dtype=torch.float32, device=DEV)
    sides = []
    for _ in range(2):
        sides.append(dict(prev=torch.rand((B, C * HW), **f32), out=torch.zeros((B, C * HW), **f32), val_prev=torch.zeros(B, **f32),
                          rewards=torch.zeros(B * T, **f32), dones=torch.zeros(B * T, **f32), deltas=torch.zeros(B * T, **f32)))
    sides[1]["prev"].copy_(sides[0]["prev"])
    vals = torch.rand((n, B), **f32)
    resets = 0
    for t in range(n):
        old.step(acts[t].data_ptr(), 1)
        _step_rules(world, new, acts[t].data_ptr(), rules)
        for p, s, by_rules in ((old_p, sides[0], False), (new_p, sides[1], True)):
            post = ops.world_post(vals[t].data_ptr(), 1, s["val_prev"], s["rewards"], s["dones"], s["deltas"], T, t % T, 0, GAMMA,
                                  world == "pong", s["prev"].data_ptr(), C * HW, s["out"].data_ptr(), C * HW, C)
            if by_rules:
                _step_rules(world, p, acts[t].data_ptr(), rules, post=post)
            else:
                p.device_step_post(t % T, 0, B, (acts[t].data_ptr(), 1), post, frames=True)
        for name in ("state", "frames", "rew", "done", "reset_mask", "ep_stats"):
            assert torch.equal(getattr(old, name), getattr(new, name)), (t, name)
            assert torch.equal(getattr(old_p, name), getattr(new_p, name)), (t, name, "post")
        for name in sides[0]:
            assert torch.equal(sides[0][name], sides[1][name]), (t, name)
        resets += int(old.reset_mask.sum())
    assert resets >= B and int(old.ep_stats[0]) >= B


# ---------------------------------------------------------------- 3. one launch equals the sequence it replaces
POST_STEPS, POST_T, POST_CFG = 48, 3, (2, 4, 1, 4)
POST_WORLDS = {"pong": NATURAL["pong"], "breakout": dict(lives=2, max_episode_steps=97)}


class _Side:
    """one pool with the rules of POST_CFG (Breakout: both flags, the planted wall) and one set of rollout buffers, rows
    addressed as in the Runner's buffers: slot0 + b, T rows per slot"""

    def __init__(self, world, B, C, recurrent):
        from a2c_amd import ops
        self.pool = _classes(world)[0](B, DEV, seed=4, **rule_kw(world, POST_CFG), **POST_WORLDS[world])
        assert self.pool.rules is not None
        self.pool.reset_all()
        if world == "breakout":
            self.pool.state[:, 11:17] = torch.tensor(PLANT_ROWS, dtype=torch.int32, device=DEV)
            self.pool.state[:, 6] = PLANTED
        self.HW, self.S, self.slot0, T = self.pool.HW, C * self.pool.HW, 2, POST_T
        N = (self.slot0 + B) * T
        f32 = dict(dtype=torch.float32, device=DEV)
        self.states = torch.zeros((N, self.S), **f32)
        self.bookmark = torch.zeros((B, self.S), **f32)
        ops.frame_stack_push(self.pool.frames, torch.ones(B, **f32), self.bookmark.data_ptr(), self.S, self.bookmark.data_ptr(),
                             self.S, B, C, self.HW)
        self.rewards, self.dones, self.deltas = (torch.full((N,), -7.0, **f32) for _ in range(3))
        self.val_prev, self.done_eff = torch.zeros(B, **f32), torch.full((B,), -7.0, **f32)
        self.h = torch.zeros((B, 5), **f32) if recurrent else None

    def sp(self, t):
        return self.states.data_ptr() + 4 * (self.slot0 * POST_T + t) * self.S

    def rows(self, t):
        if t + 1 < POST_T:
            return self.sp(t + 1), POST_T * self.S
        return self.bookmark.data_ptr(), self.S

    def tensors(self, frames):
        p = self.pool
        out = dict(state=p.state, rew=p.rew, done=p.done, reset=p.reset_mask, ep_stats=p.ep_stats, rewards=self.rewards,
                   dones=self.dones, deltas=self.deltas, val_prev=self.val_prev, states=self.states, bookmark=self.bookmark)
        if frames:
            out["frames"] = p.frames
        if self.h is not None:
            out.update(h=self.h, done_eff=self.done_eff)
        return out


@pytest.mark.parametrize("B,C,recurrent,frames", [(B, C, rec, True) for B in (1, 7, 70) for C in (1, 4) for rec in (False, True)]
                         + [(7, 4, False, False), (7, 4, True, False)])
@pytest.mark.parametrize("world", ["pong", "breakout"])
def test_step_rules_with_post_equals_the_launch_sequence(world, B, C, recurrent, frames):
    from a2c_amd import ops
    pong, T = world == "pong", POST_T
    a, b = _Side(world, B, C, recurrent), _Side(world, B, C, recurrent)      # a: the launch sequence, b: one launch
    frames0 = b.pool.frames.clone()
    acts = torch.from_numpy(action_tape(world, 2, B, POST_STEPS)).to(DEV)
    g = torch.Generator().manual_seed(B * 10 + C)
    vals = torch.randn((POST_STEPS, B, 2), generator=g).to(DEV)              # val_stride = 2
    hs = torch.randn((POST_STEPS, B, 5), generator=g).to(DEV)
    HW, S = a.HW, a.S
    seen = torch.zeros(4, dtype=torch.int64, device=DEV)      # resets, life closes, steps with R > 1, hidden rows zeroed
    for k in range(POST_STEPS):
        t = k % T
        if t == 0:       # state 0 of a slot = the bookmark
            for x in (a, b):
                x.states.view(-1, T, S)[x.slot0:, 0] = x.bookmark
        if recurrent:
            a.h.copy_(hs[k])
            b.h.copy_(hs[k])
        ap, v = (acts[k].data_ptr(), 1), vals[k]
        booked = a.pool.state[:, 10].clone()
        fr, rew, done, reset = a.pool.device_step(t, 0, B, actions=ap)          # a2c_<world>_step_rules, post = NULL
        nxt, nstride = a.rows(t)
        if recurrent:
            ops.rollout_record(rew, done, v.data_ptr(), 2, a.val_prev, a.rewards, a.dones, a.deltas, a.done_eff, a.h, B, T, t,
                               a.slot0, GAMMA, pong)
            ops.frame_stack_push(fr, reset, a.sp(t), T * S, nxt, nstride, B, C, HW)
        else:
            ops.rollout_post(rew, done, v.data_ptr(), 2, a.val_prev, a.rewards, a.dones, a.deltas, T, t, a.slot0, GAMMA, pong, fr,
                             reset, a.sp(t), T * S, nxt, nstride, B, C, HW)
        nxt, nstride = b.rows(t)
        post = ops.world_post(v.data_ptr(), 2, b.val_prev, b.rewards, b.dones, b.deltas, T, t, b.slot0, GAMMA, pong, b.sp(t), T * S,
                              nxt, nstride, C, done_eff=b.done_eff if recurrent else None, h=b.h)
        b.pool.device_step_post(t, 0, B, ap, post, frames=frames)               # a2c_<world>_step_rules with post
        ta, tb = a.tensors(frames), b.tensors(frames)
        for name in ta:
            assert torch.equal(ta[name], tb[name]), (world, B, C, k, name)
        seen[0] += (reset != 0).sum()
        if not pong:
            # a life close: a reset after which the episode-step word goes on counting; R > 1: the booked reward of a step
            # that did not close grew by more than the step's (clipped) reward
            seen[1] += ((reset != 0) & (a.pool.state[:, 9] != 0)).sum()
            seen[2] += ((reset == 0) & (a.pool.state[:, 10] - booked > 1) & (rew == 1)).sum()
        if recurrent:
            seen[3] += ((b.h == 0).all(dim=1) & (done != 0)).sum()
    if not frames:       # the pool's frame rows were left alone
        assert torch.equal(b.pool.frames, frames0)
    seen = seen.tolist()
    print(f"rules post {world} B={B} C={C}: resets, life closes, R > 1, hidden rows zeroed = {seen}")
    assert float(a.deltas[a.slot0 * T:].abs().max()) > 0 and seen[0] >= 1
    if not pong:
        assert seen[1] >= 1 and seen[2] >= 1, "a life close and a clipped reward went through the one-launch form"
    if recurrent:
        assert seen[3] >= 1
    assert (a.pool.state[:, 9 if pong else 8] > POST_STEPS).all(), "game frames were played"


# ---------------------------------------------------------------- 4. the new argument checks
@pytest.mark.parametrize("post", [False, True], ids=["plain", "post"])
@pytest.mark.parametrize("world", ["pong", "breakout"])
def test_new_err_arg_cases_leave_every_buffer_untouched(world, post):
    from a2c_amd import _lib
    lib = _lib.load()
    B, C = 2, 2
    pool = _classes(world)[0](B, DEV, seed=1, **NATURAL[world])
    pool.reset_all()
    HW = pool.HW
    f32 = dict(dtype=torch.float32, device=DEV)
    bufs = {n: torch.full((4 * C * HW + 64,), -3.0, **f32) for n in ("out", "prev", "frames")}
    bufs.update({n: torch.full((64,), -3.0, **f32) for n in ("rew", "done", "reset", "val", "val_prev", "rewards", "dones", "deltas")})
    bufs["stats"] = torch.full((64,), -3, dtype=torch.int32, device=DEV)
    acts = torch.zeros(B, dtype=torch.int64, device=DEV)
    ptr = {n: x.data_ptr() + 64 for n, x in bufs.items()}      # 16 floats of canary in front of every output
    brk = world == "breakout"

    def call(**o):
        a = dict(state=pool.state.data_ptr(), actions=acts.data_ptr(), stride=1, B=B, env0=0, frames=ptr["frames"], ld=HW,
                 rew=ptr["rew"], done=ptr["done"], reset=ptr["reset"], k=2, kmax=4, num=1, den=4, life=int(brk), clip=int(brk),
                 rules=True, world={}, post=True, t=1)
        a.update(o)
        wp = _lib.WorldPost(val=ptr["val"], val_stride=1, val_prev=ptr["val_prev"], rewards=ptr["rewards"], dones=ptr["dones"],
                            deltas=ptr["deltas"], T=3, t=a["t"], slot0=0, gamma=GAMMA, pong=0, prev=ptr["prev"], prev_stride=C * HW,
                            out=ptr["out"], out_stride=C * HW, C=C, done_eff_out=None, h=None, hdim=0)
        wr = _lib.WorldRules(a["k"], a["kmax"], a["num"], a["den"], a["life"], a["clip"])
        head = (a["state"], a["actions"], a["stride"], 0, a["B"], a["env0"], 1)
        if world == "pong":
            w = dict(dict(points=2, steps=40, num=3, den=4), **a["world"])
            head += (w["points"], w["steps"], w["num"], w["den"])
        else:
            w = dict(dict(lives=1, steps=40), **a["world"])
            head += (w["lives"], w["steps"])
        args = head + (a["frames"], a["ld"], a["rew"], a["done"], a["reset"], ptr["stats"], ptr["stats"] + 4)
        return getattr(lib, f"a2c_{world}_step_rules")(*args, ctypes.byref(wr) if a["rules"] else None,
                                                       ctypes.byref(wp) if post and a["post"] else None, None)
    state0 = pool.state.clone()
    # the rules block
    bad = [dict(rules=False), dict(kmax=1), dict(kmax=9), dict(k=4, kmax=3), dict(kmax=0), dict(kmax=-1), dict(kmax=1 << 20),
           dict(k=0, kmax=0), dict(k=9, kmax=9), dict(k=0), dict(den=0), dict(den=(1 << 16) + 1), dict(num=-1), dict(num=5),
           dict(life=2), dict(life=-1), dict(clip=2), dict(clip=-1), dict(life=1 << 8), dict(clip=3, kmax=2)]
    if not brk:      # a point closes every Pong step already and |rew| <= 1: the flags are refused, not ignored
        bad += [dict(life=1), dict(clip=1), dict(life=1, clip=1), dict(life=1, kmax=2)]
    # everything today's launchers reject, with a block that takes the new kernels and with one that takes the old ones
    for blk in (dict(), dict(kmax=2, life=0, clip=0)):
        bad += [dict(blk, **o) for o in (
            dict(state=None), dict(actions=None), dict(rew=None), dict(done=None), dict(reset=None), dict(stride=-1), dict(env0=-1),
            dict(B=0), dict(B=-1), dict(frames=ptr["frames"] + 4), dict(ld=HW - 4), dict(ld=HW + 2), dict(world=dict(steps=0)),
            dict(world=dict(steps=(1 << 24) + 1)))]
        bad += [dict(blk, **o) for o in ((dict(world=dict(points=0)), dict(world=dict(points=22)), dict(world=dict(den=0)),
                                          dict(world=dict(num=5)), dict(world=dict(num=-1))) if world == "pong" else
                                         (dict(world=dict(lives=0)), dict(world=dict(lives=6))))]
        bad += [dict(blk, **o) for o in ((dict(t=3), dict(t=-1)) if post else (dict(frames=None),))]
    for o in bad:
        assert call(**o) == -1, (world, post, o)
    torch.cuda.synchronize()
    assert torch.equal(pool.state, state0)
    for n, x in bufs.items():
        assert bool((x == -3).all()), (world, n)      # nothing ran
    # ... and the valid calls at the bounds are accepted
    assert call() == 0 and call(k=1, kmax=8) == 0 and call(k=8, kmax=8) == 0 and call(k=1, kmax=1, num=0, den=1, life=0, clip=0) == 0
    assert call(num=1 << 16, den=1 << 16) == 0
    if brk:
        assert call(life=1, clip=0) == 0 and call(life=0, clip=1) == 0
    if post:
        assert call(frames=None) == 0
    torch.cuda.synchronize()
    assert not torch.equal(pool.state, state0)
    for n in ("rew", "done", "reset"):
        assert bool((bufs[n][:16] == -3).all()) and bool((bufs[n][16 + B:] == -3).all()) and bool((bufs[n][16:16 + B] != -3).all())


# ---------------------------------------------------------------- 5. through the Runner
RUNNER_B, RUNNER_T, RUNNER_ROUNDS = 4, 6, 5
RUNNER_CFG = (2, 4, 1, 4)
# model, env_type, state shape, world: Pong episodes end inside the 30 agent steps; a Breakout ball that no paddle meets is
# lost after some 60 game frames, so a life closes a step before the episode ends at 75
RUNNER_CASES = {"fc_pong": ("FCModel", "Pong-device", (4, 80, 80), "pong", dict(points_to_win=1, max_episode_steps=45)),
                "a3c_breakout": ("A3CModel", "Breakout-device", (4, 80, 72), "breakout", dict(lives=3, max_episode_steps=75)),
                "grufc_breakout": ("GRUFCModel", "Breakout-device", (4, 80, 72), "breakout", dict(lives=3, max_episode_steps=75))}


def _runner_rows(case, which):
    """RUNNER_ROUNDS rollouts (on the graph path: eager, captured, replayed x 3) of one net on one tape of uniforms ->
    the rows after every rollout, the device pool's state and counters, the host twins"""
    import a2c_amd
    from a2c_amd.runner import HostEnvPool, Runner
    kind, env_type, ss, world, kw = RUNNER_CASES[case]
    B, T = RUNNER_B, RUNNER_T
    hyps = base_hyps(env_type=env_type, n_tsteps=T, n_rollouts=B, n_envs=B, rollout_graphs=which == "graphs")
    us = torch.rand((RUNNER_ROUNDS, T, B), generator=torch.Generator().manual_seed(3)).to(DEV)
    torch.manual_seed(5)
    net = getattr(a2c_amd.models, kind)(list(ss), N_ACT[world], h_size=64 if "FC" in kind else 256, bnorm=False)
    N = B * T
    D = dict(states=torch.zeros(N, *ss, device=DEV), deltas=torch.zeros(N, device=DEV), rewards=torch.zeros(N, device=DEV),
             dones=torch.zeros(N, device=DEV), actions=torch.zeros(N, dtype=torch.int64, device=DEV))
    if net.is_recurrent:
        D["h_states"] = torch.zeros(N, net.h_size, device=DEV)
    twins = None
    if which == "host":
        twins = [_Prepped(world, seed=12, env_id=j, **kw, **rule_kw(world, RUNNER_CFG)) for j in range(B)]
        pool = HostEnvPool(twins, frame_shape=(1,) + ss[1:])
    else:
        pool = _classes(world)[0](B, DEV, seed=12, **kw, **rule_kw(world, RUNNER_CFG))
        assert pool.rules is not None
    rnd = [0]
    rq = queue.Queue(1)
    rq.put(0.0)
    r = Runner(D, hyps, None, None, rq, env_pool=pool, uniform_fn=lambda t, Bn, env0: us[rnd[0], t, env0:env0 + Bn].contiguous())
    rows = []
    for rnd[0] in range(RUNNER_ROUNDS):
        r.rollout(net, list(range(B)), hyps)
        r.finish()
        rows.append({k: v.clone() for k, v in D.items()})
    torch.cuda.synchronize()
    made = list(getattr(r, "_dev_graphs", {}).values())
    state = None if which == "host" else (pool.state.clone(), pool.ep_stats.clone())
    return rows, state, twins, made


@pytest.mark.parametrize("case", list(RUNNER_CASES))
def test_runner_device_pool_equals_host_pool_of_twins(case):
    world = RUNNER_CASES[case][3]
    got, state, _, made = _runner_rows(case, "graphs")
    want, state_w, _, made_w = _runner_rows(case, "eager")
    host, _, twins, _ = _runner_rows(case, "host")
    log = [x for e in twins for x in e.log]
    ev = {k: sum(e.env.events.get(k, 0) for e in twins) for k in ("episode_end", "cut", "sticky", "life_close")}
    print(f"rules runner {case}: host twins {ev}, rewards {sum(1 for r, d in log if r != 0)}, graphs {made}")
    assert ev["episode_end"] >= 1 and ev["cut"] >= 1 and any(r != 0 for r, d in log)
    # one k-draw per agent step and one sticky draw per game frame were taken, beside the worlds' own draws
    assert all(e.env.draws > RUNNER_ROUNDS * RUNNER_T + e.env.steps for e in twins)
    if world == "breakout":
        # (an untrained net on grey levels up to 200 asks for one action nearly always: a kept action seldom differs from it)
        assert ev["life_close"] >= 1 and all(r in (0.0, 1.0) for r, d in log)
    else:
        assert ev["sticky"] >= 1
    assert len(made) == 1 and isinstance(made[0], torch.cuda.CUDAGraph) and not made_w      # captured; not on the comparator
    for k in range(RUNNER_ROUNDS):
        for name in want[k]:
            assert torch.equal(got[k][name], want[k][name]), (case, k, name)
        d, h = want[k], host[k]
        assert torch.equal(d["actions"], h["actions"]), k
        assert torch.equal(d["dones"], h["dones"]), k
        assert torch.equal(d["states"], h["states"]), k
        close("rewards", d["rewards"], h["rewards"].cpu().numpy(), 1e-5, 1e-5)
        close("deltas", d["deltas"], h["deltas"].cpu().numpy(), 1e-5, 1e-5)
        if "h_states" in d:
            close("h_states", d["h_states"], h["h_states"].cpu().numpy(), 1e-5, 1e-5)
    assert torch.equal(state[0], state_w[0]) and torch.equal(state[1], state_w[1])
    # the pool's words are the twins': the k-draws inside the replayed launches took the draws the twins took
    for j, e in enumerate(twins):
        words = state_w[0][j].tolist()
        if world == "pong":
            assert words[9] == e.env.steps and words[12] == e.env.prev and words[8] == e.env.draws, j
        else:
            assert np.array_equal(np.array(words, dtype=np.int32), e.env.state_words()), j
    assert int(state_w[0][:, 9 if world == "pong" else 8].min()) > RUNNER_ROUNDS * RUNNER_T


# ---------------------------------------------------------------- 6. the evaluator
def test_device_stats_runner_with_frame_skip_max():
    """DeviceStatsRunner on Pong worlds with Pong-v0's stepping rule against the twins by ACTION REPLAY: the recorded actions
    replayed on ``PongEnv``s with the same keys give the recorded rows, ep_rew, ep_len (in AGENT steps) and the result"""
    import a2c_amd
    from a2c_amd.pong import DevicePongPool, PongEnv
    from a2c_amd.runner import DeviceStatsRunner
    E, chunk, cap, seed, ID0 = 7, 4, 14, 3, 10007
    world = dict(points_to_win=1, max_episode_steps=60, **rule_kw("pong", (2, 4, 1, 4)))
    hyps = base_hyps(env_type="Pong-device", n_test_eps=E, eval_chunk=chunk, max_eval_steps=cap)
    torch.manual_seed(5)
    net = a2c_amd.models.FCModel([4, 80, 80], 3, h_size=64, bnorm=False)
    us = torch.rand((2, 16, E), generator=torch.Generator().manual_seed(0)).to(DEV)
    call = [0]
    ev = DeviceStatsRunner(hyps, DevicePongPool(E, DEV, seed=seed, **world),
                           uniform_fn=lambda t, Bn, env0: us[call[0], t, env0:env0 + Bn].contiguous(), keep_actions=True)
    ended = capped = 0
    ks = set()
    for call[0] in range(2):
        got, last = ev.rollout(net), ev.last
        acts, rews, dones = (last[k].numpy() for k in ("actions", "rewards", "dones"))
        ep_rew, ep_len, active = np.zeros(E, dtype=np.float32), np.zeros(E, dtype=np.int32), np.ones(E, dtype=np.int32)
        for j in range(E):
            e = PongEnv(seed=seed, env_id=ID0 + call[0] * E + j, **world)
            e.new_episode()
            for t in range(cap):
                assert t < acts.shape[0], "the evaluator stopped while this env was playing"
                r, d = e.advance(int(acts[t, j]))
                ks.add(e.last_k)
                done = d or r != 0
                assert rews[t, j] == r and dones[t, j] == float(done), (call[0], j, t)
                ep_rew[j] = np.float32(ep_rew[j] + np.float32(r))
                ep_len[j] += 1
                if done:
                    active[j] = 0
                    break
        print(f"rules evaluator call {call[0]}: ep_len {ep_len.tolist()} ep_rew {ep_rew.tolist()} active {active.tolist()} ks {ks}")
        assert np.array_equal(last["ep_rew"].numpy(), ep_rew) and np.array_equal(last["ep_len"].numpy(), ep_len)
        assert np.array_equal(last["active"].numpy(), active)
        assert got == float(ep_rew.astype(np.float64).sum()) / E
        ended, capped = ended + int((active == 0).sum()), capped + int((active != 0).sum())
    assert ks == {2, 3, 4} and ended >= 1, (ks, ended, capped)


# ---------------------------------------------------------------- 7. train()
def _train(tmp_path, name, on_epoch=True, **hyp):
    from a2c_amd.training import train
    hyps = dict(exp_name=name, main_path=str(tmp_path), model="FCModel", n_envs=8, n_rollouts=8, n_tsteps=5, n_frame_stack=3,
                max_tsteps=1e9, seed=1, h_size=32, n_test_eps=2, max_eval_steps=20, frame_skip=2, frame_skip_max=4, sticky_num=1,
                sticky_den=4, **hyp)
    seen = []
    best = train(None, hyps, verbose=False, max_epochs=2,
                 on_epoch=lambda epoch, upd, D: seen.append((tuple(D["states"].shape), int(D["actions"].max()),
                                                             bool(torch.isfinite(D["deltas"]).all()), float(D["dones"].sum()),
                                                             float(D["rewards"].abs().max()))))
    log = open(os.path.join(str(tmp_path), name, name + "_0", "log.txt")).read()
    assert len(seen) == 2 and seen[0][2] and seen[1][2] and np.isfinite(best)
    assert "BestRew:" in log and "frame_skip:2" in log and "frame_skip_max:4" in log and "sticky_den:4" in log
    return seen, log


def test_train_takes_the_pong_v0_keys(tmp_path):
    """``Pong-device`` with frame_skip=2, frame_skip_max=4, sticky 1/4: Pong-v0's stepping rule"""
    seen, log = _train(tmp_path, "pongv0", env_type="Pong-device", points_to_win=2, max_episode_steps=30)
    assert seen[0][0] == (40, 3, 80, 80) and 0 <= seen[0][1] < 3
    assert seen[0][3] + seen[1][3] >= 1, "10 agent steps of 2..4 game frames see a point or end a 30-frame episode"


@pytest.mark.parametrize("eval_pool", ["host", "device"])
def test_train_breakout_device_keeps_the_training_flags_out_of_evaluation(eval_pool, tmp_path, monkeypatch):
    from a2c_amd import breakout
    pools, twins = [], []

    class Pool(breakout.DeviceBreakoutPool):
        def __init__(self, *a, **kw):
            pools.append(kw)
            super().__init__(*a, **kw)
    factory = breakout.BreakoutFactory

    def recording_factory(**kw):
        twins.append(kw)
        return factory(**kw)
    monkeypatch.setattr(breakout, "DeviceBreakoutPool", Pool)
    monkeypatch.setattr(breakout, "BreakoutFactory", recording_factory)
    seen, log = _train(tmp_path, "brk", env_type="Breakout-device", eval_pool=eval_pool, lives=2, max_episode_steps=30,
                       episodic_life=True, clip_rewards=True)
    assert seen[0][0] == (40, 3, 80, 72) and 0 <= seen[0][1] < 4
    assert seen[0][3] + seen[1][3] >= 1, "10 agent steps of 2..4 game frames end a 30-frame episode"
    assert "episodic_life:True" in log and "clip_rewards:True" in log
    # the training pool has all three keys ...
    assert (pools[0]["frame_skip_max"], pools[0]["episodic_life"], pools[0]["clip_rewards"]) == (4, True, True)
    # ... the evaluation worlds the dynamics only: a whole game, the game's score
    evals = pools[1:] if eval_pool == "device" else twins
    assert len(pools) == (2 if eval_pool == "device" else 1) and len(evals) >= 1
    for kw in evals:
        assert kw["frame_skip_max"] == 4 and (kw["frame_skip"], kw["sticky_num"], kw["sticky_den"]) == (2, 1, 4), kw
        assert not kw.get("episodic_life", False) and not kw.get("clip_rewards", False), kw
    if eval_pool == "host":
        assert all(kw["env_id"] >= 10007 for kw in twins)


def test_train_breakout_host_behind_the_process_pool(tmp_path):
    seen, log = _train(tmp_path, "brkhost", env_type="Breakout-host", lives=2, max_episode_steps=30, episodic_life=True,
                       clip_rewards=True, n_env_workers=2)
    assert seen[0][0] == (40, 3, 80, 72) and 0 <= seen[0][1] < 4
    assert seen[0][3] + seen[1][3] >= 1
    assert "episodic_life:True" in log and "clip_rewards:True" in log and "env_type:Breakout-host" in log
