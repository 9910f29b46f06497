"""Frame skip and sticky actions on the host twins ``PongEnv`` / ``BreakoutEnv`` (no GPU needed): an
agent step of ``frame_skip`` = k game frames against today's twin stepped k times and cut at the real done -- an oracle
that runs none of the new code --, the sticky draws against a loop written out here from ``hash32``, the bounds, and
``skip_play``: the twins' play on every (world, B, k, sticky) tuple tests/test_gpu_world_skip.py compares the device
worlds with, where the twins ALONE must show every new rule at work before that comparison means anything."""
import functools

import numpy as np
import pytest

from cases import hashf

KS = (2, 3, 4, 8)
# (frame_skip, sticky_num, sticky_den) of the device comparison
CONFIGS = ((4, 0, 1), (3, 1, 4), (8, 1, 4), (2, 1, 1))
BS = (1, 7, 70)
N_STEPS = {1: 96, 7: 96, 70: 32}          # agent steps per pool size
PONG_STATE = ("agent_y", "opp_y", "ball_x", "ball_y", "vx", "vy", "score_agent", "score_opp", "draws", "steps", "ep_steps")
BRK_STATE = ("paddle_x", "ball_x", "ball_y", "vx", "vy", "lives_left", "bricks_left", "draws", "steps", "ep_steps", "ep_rew", "rows")
N_ACT = {"pong": 3, "breakout": 4}
# max_episode_steps = 37 is a multiple of no k in use: episodes end inside agent steps
WORLDS = {"pong": dict(points_to_win=2, max_episode_steps=37), "breakout": dict(lives=2, max_episode_steps=150)}
# the Breakout worlds of skip_play start from a wall with every other brick gone (and end after 37 game frames): a ball that
# enters a gap takes the brick above it and, on its way down, a neighbour of the gap -- two bricks within two game frames,
# which an intact wall does not give in play this short
PLANT_ROWS = (0x15555, 0x2AAAA, 0x15555, 0x2AAAA, 0x15555, 0x2AAAA)
PLAY_WORLDS = {"pong": WORLDS["pong"], "breakout": dict(lives=2, max_episode_steps=37)}
# (world, B, config) -> (seed of the worlds and of the action tape, world); chosen ON THE CPU so that the host twins alone
# show every new rule (test_every_new_rule_is_seen_on_the_host_twins) within N_STEPS[B] agent steps.  Absent: (0,
# PLAY_WORLDS).  Pong, k = 3: in the 37-frame world no point falls on the first or second frame of a step; in 70-frame
# episodes to 21 points some do
_PONG_K3 = dict(points_to_win=21, max_episode_steps=70)
SKIP_SEEDS = {("pong", 1, (3, 1, 4)): (2, _PONG_K3), ("pong", 7, (3, 1, 4)): (0, _PONG_K3), ("pong", 70, (3, 1, 4)): (0, _PONG_K3)}


def twin(world, **kw):
    from a2c_amd.breakout import BreakoutEnv
    from a2c_amd.pong import PongEnv
    return (PongEnv if world == "pong" else BreakoutEnv)(**kw)


def state_of(world, e):
    return tuple(tuple(e.rows) if k == "rows" else getattr(e, k) for k in (PONG_STATE if world == "pong" else BRK_STATE))


def action_tape(world, seed, B, n):
    """pre-drawn actions (n, B) from hashf: independent of the worlds' states"""
    A = N_ACT[world]
    return (hashf(n * B, 1000 + seed) * A).astype(np.int64).clip(0, A - 1).reshape(n, B)


def plain_agent_step(e, a, k):
    """today's world (a default twin) stepped up to k times with one action, cut at the real done"""
    total, done = 0.0, False
    for _ in range(k):
        r, done = e.advance(a)
        total += r
        if done:
            break
    return total, done


# ---------------------------------------------------------------- 1. skip equals k plain steps
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("world", ["pong", "breakout"])
def test_skip_equals_k_plain_steps(world, k):
    n, ends, cuts = 96, 0, 0
    for seed, kw in ((0, WORLDS[world]), (3, dict(WORLDS[world], max_episode_steps=37))):
        acts = action_tape(world, seed, 1, n)[:, 0]
        new, old = twin(world, seed=seed, env_id=5, frame_skip=k, **kw), twin(world, seed=seed, env_id=5, **kw)
        new.new_episode()
        old.new_episode()
        for t in range(n):
            got, want = new.advance(int(acts[t])), plain_agent_step(old, int(acts[t]), k)
            assert got == want, (seed, t, got, want)
            if want[1]:
                ends += 1
                new.new_episode()
                old.new_episode()
            assert state_of(world, new) == state_of(world, old), (seed, t)
            assert new.prev == 0 and np.array_equal(new.prepped(), old.prepped()), (seed, t)
        cuts += new.events["cut"]
        assert {k_: v for k_, v in new.events.items() if k_ not in ("cut", "sticky")} == old.events
        assert new.events["sticky"] == 0
    assert ends >= 2 and cuts >= 1, (ends, cuts)


# ---------------------------------------------------------------- 2. the sticky draws
@pytest.mark.parametrize("world,k", [("pong", 1), ("pong", 3), ("breakout", 1), ("breakout", 4)])
def test_sticky_quarter_equals_the_loop_written_out(world, k):
    """the twin with sticky 1/4 == a DEFAULT twin whose ``draws`` counter the test advances itself: before every game frame
    one hash32 draw at the counter's value decides between the requested and the previous executed action"""
    from a2c_amd.snake import hash32
    seed, env_id, n = 4, 9, 96
    kw = dict(WORLDS[world], max_episode_steps=37)
    acts = action_tape(world, seed, 1, n)[:, 0]
    new, old = twin(world, seed=seed, env_id=env_id, frame_skip=k, sticky_num=1, sticky_den=4, **kw), twin(world, seed=seed, env_id=env_id, **kw)
    new.new_episode()
    old.new_episode()
    prev, kept, ends = 0, 0, 0
    for t in range(n):
        a, total, done = int(acts[t]), 0.0, False
        for s in range(k):
            d = hash32(seed, env_id, old.draws)
            old.draws += 1
            x = prev if d % 4 < 1 else a
            kept += x != a
            prev = x
            r, done = old.advance(x)
            total += r
            if done:
                prev = 0
                break
        assert new.advance(a) == (total, done), t
        assert new.prev == prev, t
        if done:
            ends += 1
            new.new_episode()
            old.new_episode()
        assert state_of(world, new) == state_of(world, old), t
    assert kept >= 1 and new.events["sticky"] == kept and ends >= 2, (kept, new.events, ends)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("world", ["pong", "breakout"])
def test_sticky_zero_takes_no_draw(world, k):
    seed, n = 1, 60
    acts = action_tape(world, seed, 1, n)[:, 0]
    a, b = twin(world, seed=seed, frame_skip=k, sticky_num=0, sticky_den=1, **WORLDS[world]), twin(world, seed=seed, frame_skip=k, **WORLDS[world])
    c = twin(world, seed=seed, frame_skip=k, sticky_num=0, sticky_den=1 << 16, **WORLDS[world])
    for e in (a, b, c):
        e.new_episode()
    for t in range(n):
        outs = [e.advance(int(acts[t])) for e in (a, b, c)]
        assert outs[0] == outs[1] == outs[2], t
        for e in (a, b, c):
            if outs[0][1]:
                e.new_episode()
        assert state_of(world, a) == state_of(world, b) == state_of(world, c) and a.draws == b.draws and a.prev == 0, t


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("world", ["pong", "breakout"])
def test_sticky_always_never_moves_the_paddle(world, k):
    """sticky 1/1: every game frame keeps the previous action, which a reset makes 0 (stay / nothing)"""
    seed, n = 2, 96
    acts = action_tape(world, seed, 1, n)[:, 0]
    e = twin(world, seed=seed, frame_skip=k, sticky_num=1, sticky_den=1, **dict(WORLDS[world], max_episode_steps=37))
    e.new_episode()
    paddle = "agent_y" if world == "pong" else "paddle_x"
    start, ends, draws = getattr(e, paddle), 0, e.draws
    for t in range(n):
        r, done = e.advance(int(acts[t]))
        assert e.prev == 0
        if done:
            ends += 1
            e.new_episode()
        assert getattr(e, paddle) == start, t
    assert ends >= 1 and e.events["sticky"] >= 1 and e.draws >= draws + e.steps      # one sticky draw per game frame


# ---------------------------------------------------------------- 3. the twins' play the device worlds are compared with
def _probe(world, **kw):
    """a twin that keeps (reward, done) of the game frames of its last agent step in ``trace``"""
    from a2c_amd.breakout import BreakoutEnv
    from a2c_amd.pong import PongEnv

    class Probe(PongEnv if world == "pong" else BreakoutEnv):
        trace = ()

        def advance(self, action):
            self.trace = []
            return super().advance(action)

        def _frame(self, a):
            out = super()._frame(a)
            self.trace.append(out)
            return out
    return Probe(**kw)


def words_of(world, e):
    """the twin as the int32 words of the device state (Pong: 16, word 11 = the reward since the last done, always 0 after
    a step, word 12 = prev; Breakout: ``state_words()``)"""
    if world == "breakout":
        return e.state_words().astype(np.int64) & 0xFFFFFFFF
    w = np.zeros(16, dtype=np.int64)
    w[:len(PONG_STATE)] = [getattr(e, k) for k in PONG_STATE]
    w[12] = e.prev
    return w & 0xFFFFFFFF


@functools.lru_cache(maxsize=1)
def skip_play(world, B, cfg):
    """B host twins with (frame_skip, sticky_num, sticky_den) = cfg fed the action tape, restarted after a real done like
    the Runner does -> dict of acts, rew, done (Pong: the override, a non-zero reward or the real done), reset (the real
    done) (n, B); frames (n + 1, B, HW) uint8, frame 0 the reset frame, frame t + 1 what agent step t left (the reset frame
    after a real done); words (n + 1, B, W) likewise; closed (n, 2): the dones so far and the rewards they closed, after
    every agent step; events: the twins' event counts plus mid_point (points on a game frame that was not the step's last
    one, with play going on after it) and multi_brick (agent steps with more than one brick).  Left unchanged."""
    k, num, den = cfg
    seed, kw = SKIP_SEEDS.get((world, B, cfg), (0, PLAY_WORLDS[world]))
    n = N_STEPS[B]
    acts = action_tape(world, seed, B, n)
    envs = [_probe(world, seed=seed, env_id=j, frame_skip=k, sticky_num=num, sticky_den=den, **kw) for j in range(B)]
    for e in envs:
        e.new_episode()
        if world == "breakout":
            e.rows, e.bricks_left = list(PLANT_ROWS), sum(bin(m).count("1") for m in PLANT_ROWS)
    HW = envs[0].prepped().size
    frames = np.zeros((n + 1, B, HW), dtype=np.uint8)
    words = np.zeros((n + 1, B, len(words_of(world, envs[0]))), dtype=np.int64)
    rew, done, reset = (np.zeros((n, B), dtype=np.float32) for _ in range(3))
    closed = np.zeros((n, 2), dtype=np.int64)
    since = [0] * B                                  # reward since the env's last (agent-step) done
    n_closed = sum_closed = mid_point = multi_brick = 0
    for j, e in enumerate(envs):
        frames[0, j], words[0, j] = e.prepped().reshape(-1), words_of(world, e)
    for t in range(n):
        for j, e in enumerate(envs):
            r, d = e.advance(int(acts[t, j]))
            mid_point += world == "pong" and any(fr != 0 and not fd for fr, fd in e.trace[:k - 1])
            multi_brick += world == "breakout" and sum(1 for fr, fd in e.trace if fr != 0) > 1
            if d:
                e.new_episode()
            dn = d or (world == "pong" and r != 0)
            since[j] += int(r)
            if dn:
                n_closed, sum_closed, since[j] = n_closed + 1, sum_closed + since[j], 0
            frames[t + 1, j], words[t + 1, j] = e.prepped().reshape(-1), words_of(world, e)
            rew[t, j], done[t, j], reset[t, j] = r, float(dn), float(d)
        closed[t] = n_closed, sum_closed
    events = {k_: sum(e.events[k_] for e in envs) for k_ in envs[0].events}
    events.update(mid_point=int(mid_point), multi_brick=int(multi_brick))
    out = dict(acts=acts, rew=rew, done=done, reset=reset, frames=frames, words=words, closed=closed)
    for a in out.values():
        a.setflags(write=False)
    return dict(out, events=events, seed=seed, world=kw, n=n)


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "k%d_sticky%d_%d" % c)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("world", ["pong", "breakout"])
def test_every_new_rule_is_seen_on_the_host_twins(world, B, cfg):
    h = skip_play(world, B, cfg)
    ev = h["events"]
    print(f"skip play {world} B={B} cfg={cfg} seed={h['seed']} world={h['world']}: {ev}")
    assert ev["cut"] >= 1, ev
    if cfg[1] > 0:
        assert ev["sticky"] >= 1, ev
        assert (h["words"][:, :, 12 if world == "pong" else 17] != 0).any() or cfg[1] == cfg[2], "prev is never seen non-zero"
    if world == "pong":
        assert ev["mid_point"] >= 1, ev
        assert np.abs(h["rew"]).max() == 1
    else:
        assert ev["multi_brick"] >= 1, ev
    assert len(np.unique(h["acts"])) == N_ACT[world]


# ---------------------------------------------------------------- 4. bounds
def test_bounds_raise_value_error():
    from a2c_amd import breakout, pong
    bad = (dict(frame_skip=0), dict(frame_skip=9), dict(sticky_den=0), dict(sticky_den=(1 << 16) + 1), dict(sticky_num=-1),
           dict(sticky_num=2, sticky_den=1), dict(sticky_num=5, sticky_den=4))
    for mod, env, pool in ((pong, pong.PongEnv, pong.DevicePongPool), (breakout, breakout.BreakoutEnv, breakout.DeviceBreakoutPool)):
        for kw in bad:
            with pytest.raises(ValueError):
                mod.check_world(**kw)
            with pytest.raises(ValueError):
                mod.repeat_from_hyps(kw)
            with pytest.raises(ValueError):
                env(**kw)
            with pytest.raises(ValueError):
                pool(2, "cpu", **kw)                 # the bounds come before the first allocation
        assert mod.repeat_from_hyps({}) == (1, 0, 1) and mod.repeat_from_hyps(dict(frame_skip=None, sticky_num=None)) == (1, 0, 1)
        assert mod.repeat_from_hyps(dict(frame_skip=8, sticky_num=1 << 16, sticky_den=1 << 16)) == (8, 1 << 16, 1 << 16)
        assert mod.check_world(frame_skip=8, sticky_num=1, sticky_den=4) == mod.check_world()      # the return value stays
    assert pong.world_from_hyps(dict(frame_skip=4)) == (21, 10000, 3, 4)
    assert breakout.world_from_hyps(dict(frame_skip=4, sticky_num=1, sticky_den=4)) == (5, 10000)
    f = pong.PongFactory(env_id=3, frame_skip=4, sticky_num=1, sticky_den=4)()
    assert (f.frame_skip, f.sticky_num, f.sticky_den, f.env_id) == (4, 1, 4, 3)
    f = breakout.BreakoutFactory(env_id=3, frame_skip=2)()
    assert (f.frame_skip, f.sticky_num, f.sticky_den, f.env_id) == (2, 0, 1, 3)


@pytest.mark.parametrize("kw", [dict(frame_skip=2), dict(sticky_num=1, sticky_den=4), dict(frame_skip=9)])
def test_train_refuses_frame_skip_on_snake_before_the_device(kw, tmp_path, monkeypatch):
    import torch
    from a2c_amd.training import train

    def no_device(*a, **k):
        raise AssertionError("train() touched the device")
    monkeypatch.setattr(torch.Tensor, "cuda", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    hyps = dict(exp_name="snk", main_path=str(tmp_path), model="FCModel", env_type="Snake-host", env_pool="serial", n_envs=2,
                n_rollouts=2, n_tsteps=2, n_frame_stack=2, max_tsteps=1e9, seed=1, h_size=16, **kw)
    with pytest.raises(ValueError):
        train(None, hyps, verbose=False, max_epochs=1)
    assert not list(tmp_path.iterdir()), "nothing was written either"
