"""Random frame skip, episodic life and reward clipping on the host twins ``PongEnv`` / ``BreakoutEnv`` (DESIGN.md section 6i;
no GPU needed), by the method of tests/test_world_skip.py: every rule against a DEFAULT twin -- one game frame per
``advance`` -- driven from a loop written out here with ``hash32`` and that twin's ``draws`` counter, an oracle that runs
none of the new code; the bounds; and ``rules_play``: the twins' play on every (world, B, config) tuple
tests/test_gpu_world_rules.py compares the device worlds with, where the twins ALONE must show every new rule at work
before that comparison means anything."""
import functools

import numpy as np
import pytest

from test_world_skip import BRK_STATE, N_ACT, PLANT_ROWS, PONG_STATE, action_tape, state_of, twin, words_of  # noqa: F401

BS = (1, 7, 70)
# (frame_skip, frame_skip_max, sticky_num, sticky_den) of the device comparison; Breakout plays them with both flags on
CONFIGS = {"pong": ((2, 4, 1, 4), (1, 8, 0, 1)), "breakout": ((2, 4, 1, 4), (4, 4, 0, 1), (1, 8, 0, 1))}
N_STEPS = {1: 96, 7: 96, 70: 48}          # agent steps per pool size
# rules 2 and 3 alone (one game frame per agent step) need a longer play before a life close AND an episode end occur
FLAGS_ONLY, FLAGS_ONLY_B, FLAGS_ONLY_STEPS = (1, 1, 0, 1), 7, 200
# max_episode_steps = 37 / 97 are multiples of no k in use: episodes end inside agent steps
PLAY_WORLDS = {"pong": dict(points_to_win=2, max_episode_steps=37), "breakout": dict(lives=2, max_episode_steps=97)}
PLAY_SEED = 0
cfg_id = lambda c: "k%d_%d_sticky%d_%d" % c


def play_cases():
    out = [(w, B, c) for w in ("pong", "breakout") for B in BS for c in CONFIGS[w]]
    return out + [("breakout", FLAGS_ONLY_B, FLAGS_ONLY)]


def rule_kw(world, cfg, flags=True):
    """the keywords of a twin or a pool for a config (Breakout: with both flags unless ``flags`` is False)"""
    kw = dict(frame_skip=cfg[0], frame_skip_max=cfg[1], sticky_num=cfg[2], sticky_den=cfg[3])
    if world == "breakout" and flags:
        kw.update(episodic_life=True, clip_rewards=True)
    return kw


def restart(e):
    """what ``reset()`` does after a done, without the frame"""
    if e.closed:
        e.continue_episode()
    else:
        e.new_episode()


def oracle_step(old, a, cfg, prev, seed, env_id, episodic=False):
    """ONE agent step by the rules of section 6i on a DEFAULT twin ``old`` (an ``advance`` of it is one game frame): the
    k-draw first, a sticky draw before every frame, the break at an episode end or -- with ``episodic`` -- at a lost life that
    does not end the episode, where this loop also zeroes the twin's ``ep_rew`` word.
    -> (summed reward, episode ended, life close, prev, k, game frames run)"""
    from a2c_amd.worlds import hash32
    lo, hi, num, den = cfg
    k = lo
    if hi > lo:
        k = lo + hash32(seed, env_id, old.draws) % (hi - lo + 1)
        old.draws += 1
    total, done, life, ran = 0.0, False, False, 0
    for s in range(k):
        x = a
        if num > 0:
            d = hash32(seed, env_id, old.draws)
            old.draws += 1
            x = prev if d % den < num else a
            prev = x
        lives = getattr(old, "lives_left", None)
        r, done = old.advance(x)
        total, ran = total + r, ran + 1
        life = episodic and not done and old.lives_left < lives
        if life:
            old.ep_rew = 0
        if done or life:
            prev = 0
            break
    return total, done, life, prev, k, ran


# ---------------------------------------------------------------- 1. rule 1: the k-draw
@pytest.mark.parametrize("sticky", [(0, 1), (1, 4)], ids=["plain", "sticky1_4"])
@pytest.mark.parametrize("lo,hi", [(2, 4), (1, 8)])
@pytest.mark.parametrize("world", ["pong", "breakout"])
def test_random_skip_equals_the_loop_written_out(world, lo, hi, sticky):
    seed, env_id, n = 4, 9, 160
    kw = dict(PLAY_WORLDS[world], max_episode_steps=37)
    cfg = (lo, hi) + sticky
    acts = action_tape(world, seed, 1, n)[:, 0]
    new, old = twin(world, seed=seed, env_id=env_id, **rule_kw(world, cfg, flags=False), **kw), twin(world, seed=seed, env_id=env_id, **kw)
    new.new_episode()
    old.new_episode()
    prev, ends, cuts, ks = 0, 0, 0, set()
    for t in range(n):
        a = int(acts[t])
        total, done, _, prev, k, ran = oracle_step(old, a, cfg, prev, seed, env_id)
        assert new.advance(a) == (total, done), t
        assert (new.prev, new.last_k) == (prev, k), t
        ks.add(k)
        cuts += ran < k
        if done:
            ends += 1
            new.new_episode()
            old.new_episode()
        assert state_of(world, new) == state_of(world, old), t
        assert np.array_equal(new.prepped(), old.prepped()), t
    assert ks == set(range(lo, hi + 1)), ks
    assert ends >= 2 and cuts >= 1 and new.events["cut"] == cuts, (ends, cuts, new.events)


@pytest.mark.parametrize("k,sticky", [(1, (0, 1)), (4, (0, 1)), (3, (1, 4))])
@pytest.mark.parametrize("world", ["pong", "breakout"])
def test_frame_skip_max_equal_to_frame_skip_takes_no_draw(world, k, sticky):
    seed, n = 1, 60
    kw = dict(PLAY_WORLDS[world], frame_skip=k, sticky_num=sticky[0], sticky_den=sticky[1])
    acts = action_tape(world, seed, 1, n)[:, 0]
    a, b, c = twin(world, seed=seed, frame_skip_max=k, **kw), twin(world, seed=seed, **kw), twin(world, seed=seed, frame_skip_max=None, **kw)
    assert a.frame_skip_max == b.frame_skip_max == c.frame_skip_max == k
    for e in (a, b, c):
        e.new_episode()
    for t in range(n):
        outs = [e.advance(int(acts[t])) for e in (a, b, c)]
        assert outs[0] == outs[1] == outs[2], t
        for e in (a, b, c):
            if outs[0][1]:
                e.new_episode()
        assert state_of(world, a) == state_of(world, b) == state_of(world, c), t
        assert a.draws == b.draws == c.draws and a.prev == b.prev and a.last_k == k, t


# ---------------------------------------------------------------- 2. rules 2 and 3: episodic life, reward clipping
@pytest.mark.parametrize("episodic,clip", [(True, True), (True, False), (False, True)], ids=["both", "episodic", "clip"])
@pytest.mark.parametrize("cfg", [(1, 1, 0, 1), (2, 4, 1, 4), (4, 4, 0, 1)], ids=cfg_id)
def test_episodic_life_and_clipping_equal_the_loop_written_out(cfg, episodic, clip):
    seed, env_id, n = 0, 3, 400 if cfg[1] == 1 else 160
    kw = dict(lives=3, max_episode_steps=97)
    acts = action_tape("breakout", seed, 1, n)[:, 0]
    new = twin("breakout", seed=seed, env_id=env_id, episodic_life=episodic, clip_rewards=clip, **rule_kw("breakout", cfg, flags=False), **kw)
    old = twin("breakout", seed=seed, env_id=env_id, **kw)
    for e in (new, old):
        e.new_episode()
        e.rows, e.bricks_left = list(PLANT_ROWS), sum(bin(m).count("1") for m in PLANT_ROWS)
    prev, since, ends, closes, big = 0, 0, 0, 0, 0
    for t in range(n):
        a = int(acts[t])
        before = (old.bricks_left, old.lives_left, old.ep_steps)
        total, done, life, prev, k, ran = oracle_step(old, a, cfg, prev, seed, env_id, episodic)
        since += int(total)
        rew, d = new.advance(a)
        assert rew == (float(np.sign(total)) if clip else total) and d == (done or life), t
        assert (new.prev, new.last_k, new.closed, new.over) == (prev, k, life, done), t
        big += abs(total) > 1
        if life:
            # the game goes on: only the frames run moved the world, and the life is gone
            assert new.lives_left == before[1] - 1 >= 1 and new.ep_steps == before[2] + ran and new.ep_rew == 0, t
            assert new.rows == old.rows and new.bricks_left == old.bricks_left <= before[0], t
            closes += 1
            words, draws, frame = new.state_words(), new.draws, new.render_rgb()
            with pytest.raises(RuntimeError):
                new.advance(a)
            assert np.array_equal(new.reset(), frame), "the continuing reset returns the current frame"
            assert np.array_equal(new.state_words(), words) and new.draws == draws and not new.closed, t
            with pytest.raises(RuntimeError):
                new.continue_episode()
            since = 0
        elif done:
            ends += 1
            new.reset()
            old.new_episode()
            for e in (new, old):      # every episode of this test starts from the planted wall
                e.rows, e.bricks_left = list(PLANT_ROWS), sum(bin(m).count("1") for m in PLANT_ROWS)
            since = 0
        else:
            assert new.ep_rew == since, "ep_rew books the unclipped reward since the last close"
        assert state_of("breakout", new) == state_of("breakout", old), t
        assert np.array_equal(new.prepped(), old.prepped()), t
    assert ends >= 1 and big >= (cfg[1] > 1), (ends, big)
    if episodic:
        assert closes >= 2 and new.events["life_close"] == closes, (closes, new.events)
    else:
        assert closes == 0 and "life_close" not in new.events


def test_new_episode_after_a_life_close_is_the_full_restart():
    e = twin("breakout", seed=0, env_id=3, lives=3, max_episode_steps=500, episodic_life=True)
    e.new_episode()
    while not e.closed:
        e.advance(0)
    assert e.lives_left == 2 and not e.over
    draws = e.draws
    e.new_episode()
    assert (e.lives_left, e.ep_steps, e.closed, e.draws) == (3, 0, False, draws + 1)
    e.advance(0)


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


@functools.lru_cache(maxsize=1)
def rules_play(world, B, cfg):
    """B host twins with ``rule_kw(world, cfg)`` fed the action tape, restarted after a done the way ``reset()`` does
    (continued after a life close) -> dict of acts, rew (Breakout: clipped), done (Pong: the override, a non-zero reward or
    the real done; Breakout: the real done or a life close), reset (Pong: the real done; Breakout: done) (n, B); ks (n, B):
    the game frames each agent step was to play; frames (n + 1, B, HW) uint8, frame 0 the start, frame t + 1 what agent step
    t left; words (n + 1, B, W) likewise; closed (n, 2): the dones so far and the UNCLIPPED rewards they closed, after every
    agent step; events: the twins' counts plus mid_point (Pong: points on a game frame that was not the step's last one, with
    play going on), life_cut / end_cut (life closes / episode ends that dropped game frames) and big (agent steps with a
    summed reward above 1, of which ``max_R`` is the largest).  Left unchanged."""
    n = FLAGS_ONLY_STEPS if cfg == FLAGS_ONLY else N_STEPS[B]
    seed, kw = PLAY_SEED, PLAY_WORLDS[world]
    acts = action_tape(world, seed, B, n)
    envs = [_probe(world, seed=seed, env_id=j, **rule_kw(world, cfg), **kw) for j in range(B)]
    for e in envs:
        e.new_episode()
        if world == "breakout":
            e.rows, e.bricks_left = list(PLANT_ROWS), sum(bin(m).count("1") for m in PLANT_ROWS)
    HW = envs[0].prepped().size
    frames = np.zeros((n + 1, B, HW), dtype=np.uint8)
    words = np.zeros((n + 1, B, len(words_of(world, envs[0]))), dtype=np.int64)
    rew, done, reset = (np.zeros((n, B), dtype=np.float32) for _ in range(3))
    ks = np.zeros((n, B), dtype=np.int64)
    closed = np.zeros((n, 2), dtype=np.int64)
    since = [0] * B                                  # unclipped reward since the env's last (agent-step) done
    n_closed = sum_closed = mid_point = life_cut = end_cut = big = max_R = ends = 0
    for j, e in enumerate(envs):
        frames[0, j], words[0, j] = e.prepped().reshape(-1), words_of(world, e)
    for t in range(n):
        for j, e in enumerate(envs):
            r, d = e.advance(int(acts[t, j]))
            R = int(sum(fr for fr, fd in e.trace))
            ks[t, j] = e.last_k
            mid_point += world == "pong" and any(fr != 0 and not fd for fr, fd in e.trace[:e.last_k - 1])
            life_cut += e.closed and len(e.trace) < e.last_k
            end_cut += e.over and len(e.trace) < e.last_k
            ends += e.over
            big, max_R = big + (R > 1), max(max_R, R)
            real = e.over
            if d:
                restart(e)
            dn = d or (world == "pong" and r != 0)
            since[j] += R
            if dn:
                n_closed, sum_closed, since[j] = n_closed + 1, sum_closed + since[j], 0
            frames[t + 1, j], words[t + 1, j] = e.prepped().reshape(-1), words_of(world, e)
            rew[t, j], done[t, j], reset[t, j] = r, float(dn), float(real if world == "pong" else d)
        closed[t] = n_closed, sum_closed
    events = {k_: sum(e.events[k_] for e in envs) for k_ in envs[0].events}
    events.update(mid_point=int(mid_point), life_cut=int(life_cut), end_cut=int(end_cut), big=int(big), max_R=int(max_R), ends=int(ends))
    out = dict(acts=acts, rew=rew, done=done, reset=reset, ks=ks, frames=frames, words=words, closed=closed)
    for a in out.values():
        a.setflags(write=False)
    return dict(out, events=events, seed=seed, world=kw, n=n)


def assert_every_rule_is_seen(world, cfg, h):
    """on the host twins alone"""
    ev = h["events"]
    assert set(np.unique(h["ks"]).tolist()) == set(range(cfg[0], cfg[1] + 1)), np.unique(h["ks"])
    if cfg[2] > 0:
        assert ev["sticky"] >= 1, ev
    if world == "pong":
        assert ev["cut"] >= 1 and ev["mid_point"] >= 1 and np.abs(h["rew"]).max() == 1, ev
        return
    assert ev["life_close"] >= 1 and ev["ends"] >= 1, ev
    assert np.abs(h["rew"]).max() == 1 and ev["big"] >= 1 and h["closed"][-1, 0] >= 2, "clipped rewards of steps with R > 1"
    if cfg[1] > 1:
        assert ev["life_cut"] >= 1 and ev["end_cut"] >= 1, ev
        assert ev["cut"] == ev["life_cut"] + ev["end_cut"], ev


@pytest.mark.parametrize("world,B,cfg", play_cases(), ids=lambda v: cfg_id(v) if isinstance(v, tuple) else str(v))
def test_every_new_rule_is_seen_on_the_host_twins(world, B, cfg):
    h = rules_play(world, B, cfg)
    print(f"rules play {world} B={B} cfg={cfg} seed={h['seed']} world={h['world']}: {h['events']}")
    assert_every_rule_is_seen(world, cfg, h)
    assert len(np.unique(h["acts"])) == N_ACT[world]


# ---------------------------------------------------------------- 4. bounds
def test_bounds_raise_value_error():
    from a2c_amd import breakout, pong, worlds
    bad = (dict(frame_skip_max=0), dict(frame_skip_max=9), dict(frame_skip=4, frame_skip_max=3), dict(frame_skip_max=-1),
           dict(frame_skip=9, frame_skip_max=9))
    bad_flags = (dict(episodic_life=2), dict(clip_rewards=-1), dict(episodic_life="yes"), dict(clip_rewards=0.5))
    for mod, env, pool in ((pong, pong.PongEnv, pong.DevicePongPool), (breakout, breakout.BreakoutEnv, breakout.DeviceBreakoutPool)):
        for kw in bad + (bad_flags if mod is breakout else ()):
            with pytest.raises(ValueError):
                mod.check_world(**kw)
            with pytest.raises(ValueError):
                mod.rules_from_hyps(kw)
            with pytest.raises(ValueError):
                env(**kw)
            with pytest.raises(ValueError):
                pool(2, "cpu", **kw)                 # the bounds come before the first allocation
        for kw in bad:
            with pytest.raises(ValueError):
                mod.repeat_from_hyps(kw)
        assert mod.repeat_from_hyps(dict(frame_skip=2, frame_skip_max=4)) == (2, 0, 1)      # the return value stays
        assert mod.check_world(frame_skip=2, frame_skip_max=8) == mod.check_world()
        assert mod.rules_from_hyps(dict(frame_skip=3))["frame_skip_max"] == 3
        assert mod.rules_from_hyps(dict(frame_skip=2, frame_skip_max=8))["frame_skip_max"] == 8
        assert mod.rules_from_hyps(dict(frame_skip=2, frame_skip_max=None, episodic_life=None, clip_rewards=False))["frame_skip_max"] == 2
    assert pong.rules_from_hyps({}) == dict(frame_skip_max=1)
    assert breakout.rules_from_hyps({}) == dict(frame_skip_max=1, episodic_life=False, clip_rewards=False)
    assert breakout.rules_from_hyps(dict(episodic_life=1, clip_rewards=True)) == dict(frame_skip_max=1, episodic_life=True, clip_rewards=True)
    # Pong closes at every point and |R| <= 1: the two Breakout keys are refused, not ignored
    for kw in (dict(episodic_life=True), dict(clip_rewards=1)):
        with pytest.raises(ValueError):
            pong.rules_from_hyps(kw)
        with pytest.raises(ValueError):
            worlds.check_rules(what="Pong", **kw)
        with pytest.raises(TypeError):
            pong.PongEnv(**kw)
        with pytest.raises(TypeError):
            pong.DevicePongPool(2, "cpu", **kw)
    for kw in (dict(frame_skip_max=1), dict(episodic_life=True), dict(clip_rewards=True)):
        with pytest.raises(ValueError):
            worlds.rules_from_hyps(kw, "Snake", ())
    assert worlds.rules_from_hyps(dict(episodic_life=False, clip_rewards=None), "Snake", ()) == {}
    f = breakout.BreakoutFactory(env_id=3, frame_skip=2, frame_skip_max=4, episodic_life=True, clip_rewards=True)()
    assert (f.frame_skip, f.frame_skip_max, f.episodic_life, f.clip_rewards, f.env_id) == (2, 4, True, True, 3)
    f = pong.PongFactory(env_id=3, frame_skip=2, frame_skip_max=4, sticky_num=1, sticky_den=4)()
    assert (f.frame_skip, f.frame_skip_max, f.env_id) == (2, 4, 3)


def test_pools_keep_the_old_entry_points_at_the_defaults():
    """the ``plain`` pattern: a pool whose new keys are all at their defaults holds no rules block"""
    from a2c_amd import ops
    assert ops.world_rules(4, 1, 4) is None and ops.world_rules(4, 1, 4, frame_skip_max=4) is None
    r = ops.world_rules(2, 1, 4, 4, True, False)
    assert (r.frame_skip, r.frame_skip_max, r.sticky_num, r.sticky_den, r.episodic_life, r.clip_rewards) == (2, 4, 1, 4, 1, 0)
    r = ops.world_rules(always=True)
    assert (r.frame_skip, r.frame_skip_max, r.sticky_num, r.sticky_den, r.episodic_life, r.clip_rewards) == (1, 1, 0, 1, 0, 0)


@pytest.mark.parametrize("env_type,kw", [("Snake-host", dict(frame_skip_max=1)), ("Snake-host", dict(episodic_life=True)),
                                         ("Snake-device", dict(clip_rewards=True)), ("Pong-host", dict(episodic_life=True)),
                                         ("Pong-device", dict(clip_rewards=True)), ("Pong-host", dict(frame_skip=4, frame_skip_max=2)),
                                         ("Breakout-device", dict(frame_skip_max=9)), ("Breakout-host", dict(episodic_life=3))])
def test_train_refuses_the_keys_before_the_device(env_type, kw, tmp_path, monkeypatch):
    import torch
    from a2c_amd.training import train

    def no_device(*a, **k):
        raise AssertionError("train() touched the device")
    monkeypatch.setattr(torch.Tensor, "cuda", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    hyps = dict(exp_name="rules", main_path=str(tmp_path), model="FCModel", env_type=env_type, env_pool="serial", n_envs=2,
                n_rollouts=2, n_tsteps=2, n_frame_stack=2, max_tsteps=1e9, seed=1, h_size=16, **kw)
    with pytest.raises(ValueError):
        train(None, hyps, verbose=False, max_epochs=1)
    assert not list(tmp_path.iterdir()), "nothing was written either"
