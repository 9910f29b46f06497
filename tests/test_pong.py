"""Pong on the host (no GPU needed): the rules of ``a2c_amd.pong.PongEnv`` on hand-built positions,
its raw frames through the reference's ``pong_prep``, determinism of the counter-based draws, the bounds of the world
parameters, and the env behind the host pools.  The device worlds are compared with this host twin, value for value, in
test_gpu_pong.py."""
import pickle

import numpy as np
import pytest

from a2c_amd import pong, preprocessing
from a2c_amd.pong import HIT_SPEED, HIT_VY, PongEnv, PongFactory, world_from_hyps
from a2c_amd.runner import HostEnvPool, SequentialEnvironment
from a2c_amd.snake import hash32

STAY, UP, DOWN = 0, 1, 2


class AlwaysMoves:
    """an opponent that moves on every step / never: opp_skill 1/1 and 0/1"""
    ON, OFF = dict(opp_skill_num=1, opp_skill_den=1), dict(opp_skill_num=0, opp_skill_den=1)


def position(ball=(39, 39), vel=(1, 0), agent_y=36, opp_y=36, scores=(0, 0), ep_steps=0, **kw):
    """an env in a hand-built position; the opponent stands still unless asked otherwise"""
    kw = dict(AlwaysMoves.OFF, **kw)
    env = PongEnv(**kw)
    env.reset()
    env.ball_x, env.ball_y = ball
    env.vx, env.vy = vel
    env.agent_y, env.opp_y = agent_y, opp_y
    env.score_agent, env.score_opp = scores
    env.ep_steps = ep_steps
    return env


# ---------------------------------------------------------------- surface
def test_surface_and_reset():
    env = PongEnv(seed=3, env_id=1)
    assert env.action_space.n == 3
    with pytest.raises(RuntimeError):
        env.step(0)                               # a new env is reset by its caller, like a gym env
    f = env.reset()
    assert f.shape == (210, 160, 3) and f.dtype == np.uint8
    assert (env.agent_y, env.opp_y, env.ball_x, env.ball_y) == (36, 36, 39, 39)
    d = hash32(3, 1, 0)
    assert env.vx == (1 if d & 1 else -1) and env.vy == (d >> 1) % 5 - 2 and env.draws == 1
    assert (env.score_agent, env.score_opp, env.ep_steps) == (0, 0, 0)


def test_the_constants_are_the_documented_ones():
    assert (pong.OPP_X, pong.AGENT_X, pong.PADDLE_W, pong.PADDLE_H, pong.BALL) == (8, 70, 2, 8, 2)
    assert HIT_VY == (-2, -2, -1, -1, 0, 1, 1, 2, 2) and HIT_SPEED == (2, 2, 1, 1, 1, 1, 1, 2, 2)
    assert (pong.MISS_LEFT, pong.MISS_RIGHT) == (6, 72)


# ---------------------------------------------------------------- the rules, on hand-built positions
@pytest.mark.parametrize("y, vy, want_y, want_vy", [(1, -2, 1, 2), (0, -1, 1, 1), (1, -1, 0, -1), (77, 2, 77, -2),
                                                    (78, 1, 77, -1), (77, 1, 78, 1), (78, 2, 76, -2), (0, -2, 2, 2)])
def test_wall_bounce(y, vy, want_y, want_vy):
    env = position(ball=(30, y), vel=(1, vy))
    _, rew, done, _ = env.step(STAY)
    assert (rew, done) == (0.0, False)
    assert (env.ball_x, env.ball_y, env.vx, env.vy) == (31, want_y, 1, want_vy)
    assert env.events["wall"] == (1 if want_vy != vy else 0)


@pytest.mark.parametrize("off", range(9))
@pytest.mark.parametrize("speed", [1, 2])
def test_agent_paddle_hit_with_each_table_entry(off, speed):
    ay = 30
    y = ay - 1 + off                              # off = ball y + 1 - paddle y
    env = position(ball=(69 - speed, y), vel=(speed, 0), agent_y=ay)
    _, rew, done, _ = env.step(STAY)
    assert (rew, done) == (0.0, False)
    assert (env.ball_x, env.ball_y) == (68, y), "the ball rests against the paddle's face"
    assert (env.vx, env.vy) == (-HIT_SPEED[off], HIT_VY[off])
    assert env.events["hit_agent"] == 1


@pytest.mark.parametrize("off", range(9))
@pytest.mark.parametrize("speed", [1, 2])
def test_opponent_paddle_hit_with_each_table_entry(off, speed):
    oy = 50
    y = oy - 1 + off
    env = position(ball=(9 + speed, y), vel=(-speed, 0), opp_y=oy)
    _, rew, done, _ = env.step(STAY)
    assert (rew, done) == (0.0, False)
    assert (env.ball_x, env.ball_y) == (10, y)
    assert (env.vx, env.vy) == (HIT_SPEED[off], HIT_VY[off])
    assert env.events["hit_opp"] == 1


def test_the_paddle_moves_before_the_ball_is_judged():
    # the ball arrives one row above the paddle's reach; moving up (2 pixels) in the same step catches it
    env = position(ball=(68, 27), vel=(1, 0), agent_y=30)
    env.step(STAY)
    assert env.events["hit_agent"] == 0 and env.ball_x == 69
    env = position(ball=(68, 27), vel=(1, 0), agent_y=30)
    env.step(UP)
    assert env.events["hit_agent"] == 1 and env.agent_y == 28 and env.vy == HIT_VY[27 + 1 - 28]


@pytest.mark.parametrize("speed", [1, 2])
def test_agent_miss_scores_for_the_opponent_and_serves_towards_the_agent(speed):
    env = position(ball=(68, 10), vel=(speed, 0), agent_y=40, seed=5, env_id=2)
    rews = []
    for _ in range(4):
        d0 = env.draws
        _, rew, done, _ = env.step(STAY)
        rews.append(rew)
        assert not done
        if rew:
            break
    assert rews[-1] == -1.0 and set(rews[:-1]) <= {0.0} and env.events["hit_agent"] == 0
    assert len(rews) == (4 if speed == 1 else 2)          # x: 68 -> 72 is the first position past the paddle's columns
    assert (env.score_agent, env.score_opp) == (0, 1)
    serve = hash32(5, 2, d0 + 1)                           # the step's opponent draw, then the serve draw
    assert (env.ball_x, env.ball_y, env.vx, env.vy) == (39, 39, 1, (serve >> 1) % 5 - 2) and env.draws == d0 + 2


@pytest.mark.parametrize("speed", [1, 2])
def test_opponent_miss_scores_for_the_agent_and_serves_towards_the_opponent(speed):
    env = position(ball=(10, 70), vel=(-speed, 0), opp_y=10, seed=5, env_id=3)
    rews = []
    for _ in range(4):
        d0 = env.draws
        _, rew, done, _ = env.step(STAY)
        rews.append(rew)
        if rew:
            break
    assert rews[-1] == 1.0 and set(rews[:-1]) <= {0.0} and not done
    assert len(rews) == (4 if speed == 1 else 2)          # x: 10 -> 6
    assert (env.score_agent, env.score_opp) == (1, 0)
    serve = hash32(5, 3, d0 + 1)
    assert (env.ball_x, env.ball_y, env.vx, env.vy) == (39, 39, -1, (serve >> 1) % 5 - 2)


def test_agent_paddle_moves_two_pixels_and_clamps_at_both_edges():
    env = position(agent_y=3)
    ys = []
    for a in (UP, UP, UP, DOWN, STAY, 3 + UP, -1):        # actions are taken mod 3: 4 is up, -1 is down
        env.ball_x, env.vx = 39, 1                        # keep the ball in mid field
        env.step(a)
        ys.append(env.agent_y)
    assert ys == [1, 0, 0, 2, 2, 0, 2]
    env = position(agent_y=69)
    for want in (71, 72, 72, 70):
        env.ball_x, env.vx = 39, 1
        env.step(DOWN if want != 70 else UP)
        assert env.agent_y == want


def test_opponent_tracks_the_ball_by_one_pixel_when_the_draw_allows():
    env = position(ball=(39, 10), vel=(0, 0), opp_y=36, **AlwaysMoves.ON)
    env.vx = 1
    for want in (35, 34):
        env.ball_x = 39
        env.step(STAY)
        assert env.opp_y == want
    env = position(ball=(39, 76), vel=(1, 0), opp_y=71, **AlwaysMoves.ON)
    for want in (72, 72):                                 # clamped at the bottom edge
        env.ball_x = 39
        env.step(STAY)
        assert env.opp_y == want
    env = position(ball=(39, 3), vel=(1, 0), opp_y=0, **AlwaysMoves.ON)      # ball centre 4 == paddle centre 4: stays
    env.step(STAY)
    assert env.opp_y == 0
    env = position(ball=(39, 0), vel=(1, 0), opp_y=1, **AlwaysMoves.ON)
    env.step(STAY)
    env.ball_x = 39
    env.step(STAY)
    assert env.opp_y == 0                                 # clamped at the top edge
    # the fraction: a 3/4 opponent moves on the steps whose draw mod 4 is below 3
    env = position(ball=(39, 10), vel=(1, 0), opp_y=60, seed=9, env_id=4, opp_skill_num=3, opp_skill_den=4)
    moved = []
    for _ in range(40):
        env.ball_x, env.ball_y, env.vy = 39, 10, 0
        d, y0 = hash32(9, 4, env.draws), env.opp_y
        env.step(STAY)
        moved.append(env.opp_y != y0)
        assert (env.opp_y == y0 - 1) == (d % 4 < 3)
    assert 0 < sum(moved) < 40


def test_points_to_win_reached_is_a_real_done():
    env = position(ball=(71, 10), vel=(1, 0), agent_y=40, scores=(0, 1), points_to_win=2)
    d0 = env.draws
    _, rew, done, _ = env.step(STAY)
    assert (rew, done) == (-1.0, True) and env.score_opp == 2 and env.draws == d0 + 1      # no serve: the caller resets
    with pytest.raises(RuntimeError):
        env.step(STAY)
    env.reset()
    assert (env.score_agent, env.score_opp, env.ep_steps) == (0, 0, 0) and env.draws == d0 + 2
    env = position(ball=(7, 10), vel=(-1, 0), opp_y=40, scores=(20, 20))
    _, rew, done, _ = env.step(STAY)
    assert (rew, done) == (1.0, True) and env.score_agent == 21
    env = position(ball=(7, 10), vel=(-1, 0), opp_y=40, scores=(19, 20))
    _, rew, done, _ = env.step(STAY)
    assert (rew, done) == (1.0, False)


def test_max_episode_steps_is_a_real_done():
    env = position(max_episode_steps=5)
    out = [env.step(STAY)[1:3] for _ in range(5)]
    assert out == [(0.0, False)] * 4 + [(0.0, True)]
    env.reset()
    assert env.ep_steps == 0 and env.steps == 5
    assert [env.step(STAY)[2] for _ in range(5)] == [False] * 4 + [True]


# ---------------------------------------------------------------- frames
def rectangles_mask(env):
    want = np.zeros((80, 80), dtype=np.uint8)
    for x, y, w, h in ((8, env.opp_y, 2, 8), (70, env.agent_y, 2, 8), (env.ball_x, env.ball_y, 2, 2)):
        want[y:y + h, x:x + w] = 1
    return want


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_pong_prep_of_the_raw_frame_is_the_prepped_frame(seed):
    env = PongEnv(seed=seed, env_id=seed + 1, points_to_win=2)
    raw = env.reset()
    for t in range(200):
        y = preprocessing.pong_prep(raw)
        assert y.shape == (1, 80, 80) and y.dtype == np.uint8
        np.testing.assert_array_equal(y, env.prepped())
        np.testing.assert_array_equal(y[0], rectangles_mask(env))
        assert 16 + 16 <= int(y.sum()) <= 16 + 16 + 4
        raw, rew, done, _ = env.step(hash32(seed, 77, t) % 3)
        if done:
            raw = env.reset()
    assert sum(env.events[k] for k in ("agent_point", "opp_point")) > 0


def test_raw_frame_layout():
    env = position(ball=(20, 5), agent_y=0, opp_y=72)
    raw = env.render_rgb()
    assert set(np.unique(raw[:35, :, 0])) == {109} and set(np.unique(raw[195:, :, 0])) == {109}
    field = raw[35:195]
    assert tuple(field[0, 0]) == (144, 72, 17)
    assert (field[10:14, 40:44] == np.array(pong.BALL_RGB)).all()               # 2 x scale
    assert (field[0:16, 140:144] == np.array(pong.AGENT_RGB)).all() and (field[144:160, 16:20] == np.array(pong.OPP_RGB)).all()
    assert (field[:, :, 0] != 144).sum() == 4 * (16 + 16 + 4)


# ---------------------------------------------------------------- randomness
def play(env, n, tape_seed=0):
    out = [env.reset().copy()]
    rews = []
    for t in range(n):
        obs, rew, done, _ = env.step(hash32(tape_seed, 0, t) % 3)
        if done:
            obs = env.reset()
        out.append(env.prepped().copy())
        rews.append((rew, done))
    return out, rews


def test_same_seed_and_env_id_give_the_same_trajectory():
    a, ra = play(PongEnv(seed=21, env_id=3, points_to_win=1), 400)
    b, rb = play(PongEnv(seed=21, env_id=3, points_to_win=1), 400)
    assert ra == rb and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert any(r for r, _ in ra) and any(d for _, d in ra)


def test_different_env_ids_and_seeds_get_different_worlds():
    a, ra = play(PongEnv(seed=21, env_id=0), 300)
    b, rb = play(PongEnv(seed=21, env_id=1), 300)
    c, rc = play(PongEnv(seed=22, env_id=0), 300)
    assert not all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not all(np.array_equal(x, y) for x, y in zip(a, c))
    serves = {(e.vx, e.vy) for e in (PongEnv(seed=21, env_id=j) for j in range(32)) if e.reset() is not None}
    assert len(serves) >= 6                               # of the 10 possible (direction, vy) pairs


def test_no_rally_runs_for_ever():
    env = PongEnv(seed=1, env_id=0, max_episode_steps=50, opp_skill_num=1, opp_skill_den=1)
    env.reset()
    n = 0
    while not env.step(STAY)[2]:
        n += 1
    assert n + 1 <= 50


# ---------------------------------------------------------------- bounds
def test_world_from_hyps_bounds():
    assert world_from_hyps({}) == (21, 10000, 3, 4)
    assert world_from_hyps(dict(points_to_win=1, max_episode_steps=1, opp_skill_num=0, opp_skill_den=1)) == (1, 1, 0, 1)
    assert world_from_hyps(dict(points_to_win=None, opp_skill_num=4)) == (21, 10000, 4, 4)
    for bad in (dict(points_to_win=0), dict(points_to_win=22), dict(max_episode_steps=0), dict(max_episode_steps=(1 << 24) + 1),
                dict(opp_skill_den=0), dict(opp_skill_num=-1), dict(opp_skill_num=5), dict(opp_skill_den=(1 << 16) + 1)):
        with pytest.raises(ValueError):
            world_from_hyps(bad)
        with pytest.raises(ValueError):
            PongEnv(**bad)


# ---------------------------------------------------------------- behind the host pools
def test_pong_env_behind_sequential_environment_and_host_pool():
    mk = lambda j: SequentialEnvironment("Pong-host", preprocessing.pong_prep, env_fn=PongFactory(seed=2, env_id=j))
    env = mk(0)
    assert env.is_discrete and env.n == 3 and env.raw_shape == (210, 160, 3)
    obs = env.reset()
    assert obs.shape == (1, 80, 80) and obs.dtype == np.uint8 and set(np.unique(obs)) == {0, 1}
    pool = HostEnvPool([mk(j) for j in range(3)], frame_shape=(1, 80, 80))
    assert len(pool) == 3 and pool.reset(1).shape == (1, 80, 80)
    obs, rew, done = pool.step(1, 2)
    assert obs.shape == (1, 80, 80) and rew in (-1.0, 0.0, 1.0) and isinstance(done, bool)
    f = pickle.loads(pickle.dumps(PongFactory(env_id=4, seed=2, points_to_win=3)))      # travels to the env workers
    assert f().env_id == 4 and f().points_to_win == 3


def test_pong_env_behind_the_process_pool_with_the_packed_transport():
    """what train(env_type="Pong-host") builds without env_pool="serial": worker processes stepping PongEnvs through
    pong_prep, the {0, 1} frames crossing the pinned region one bit per pixel, done = the real done (the reset)"""
    from a2c_amd.hostpool import FRAME_BITS, ProcessEnvPool
    B, K = 3, 50
    world = dict(seed=4, points_to_win=1, max_episode_steps=30)
    kws = [dict(env_type="Pong-host", preprocessor=preprocessing.pong_prep, seed=4, env_fn=PongFactory(env_id=j, **world))
           for j in range(B)]
    pool = ProcessEnvPool(SequentialEnvironment, B, env_kwargs=kws, n_workers=2, pong=True, register=False, frame_bits=True)
    refs = [SequentialEnvironment(**kw) for kw in kws]
    try:
        pool.start()
        pool.set_phase(1)
        h = pool.header
        assert h.frame_dtype == FRAME_BITS and h.frame_bytes == 800 and h.frame_elems == 6400
        pool.wait_frames(0)
        for j in range(B):
            assert np.array_equal(pool.frames_view()[j].reshape(1, 80, 80), refs[j].reset())
        rew, done = np.zeros(B, np.float32), np.zeros(B, np.float32)
        n_done = 0
        for k in range(K):
            acts = np.array([hash32(4, 50 + j, k) % 3 for j in range(B)], np.int64)
            pool.post_actions(acts, seq=k)
            pool.wait_frames(k + 1)
            pool.unpack(rew, done)
            fr = pool.frames_view()
            for j in range(B):
                o, r, d, _ = refs[j].step(int(acts[j]))
                if d:
                    o = refs[j].reset()
                assert np.array_equal(fr[j].reshape(1, 80, 80), o), (k, j)
                assert rew[j] == np.float32(r) and done[j] == float(d), (k, j)
                n_done += d
        assert n_done >= B
    finally:
        pool.close()
