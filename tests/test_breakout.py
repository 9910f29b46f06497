"""Breakout on the host (no GPU needed): the rules of ``a2c_amd.breakout.BreakoutEnv`` on hand-built
positions, its raw frames through the reference's ``breakout_prep``, determinism of the counter-based draws, the bounds of
the world parameters, the state words, and the env behind the host pools.  The device worlds are compared with this host
twin, value for value, in test_gpu_breakout.py."""
import pickle

import numpy as np
import pytest

from a2c_amd import breakout, preprocessing
from a2c_amd.breakout import FULL_ROW, HIT_VX, ROW_LEVEL, ROW_POINTS, BreakoutEnv, BreakoutFactory, world_from_hyps
from a2c_amd.runner import HostEnvPool, SequentialEnvironment
from a2c_amd.snake import hash32

NOOP, FIRE, RIGHT, LEFT = 0, 1, 2, 3
NO_EVENTS = dict(side_wall=0, ceiling=0, brick=0, speed_up=0, paddle_hit=0, life_lost=0, cleared=0, episode_end=0)


def position(ball=(30, 50), vel=(1, 1), px=32, lives_left=None, rows=None, ep_steps=0, **kw):
    """an env in a hand-built position (``rows``: the six brick-row masks, default the full wall)"""
    env = BreakoutEnv(**kw)
    env.reset()
    env.ball_x, env.ball_y = ball
    env.vx, env.vy = vel
    env.paddle_x = px
    if lives_left is not None:
        env.lives_left = lives_left
    if rows is not None:
        env.rows = list(rows)
        env.bricks_left = sum(bin(m).count("1") for m in rows)
    env.ep_steps = ep_steps
    return env


def events(env, **want):
    return env.events == dict(NO_EVENTS, **want)


def tracking_action(env, tape_seed, j, t):
    """the scripted policy of the parity tests: on three steps out of four the paddle follows the ball (its centre to within
    a pixel of the ball's), on the fourth the action is a random one of the four"""
    h = hash32(tape_seed ^ 0xB0, 1000 + j, t)
    if h % 4 == 0:
        return (h >> 8) % 4
    d = (env.ball_x + 1) - (env.paddle_x + 4)
    return RIGHT if d > 1 else (LEFT if d < -1 else NOOP)


# ---------------------------------------------------------------- surface
def test_surface_and_reset():
    env = BreakoutEnv(seed=3, env_id=1)
    assert env.action_space.n == 4
    with pytest.raises(RuntimeError):
        env.step(0)                               # a new env is reset by its caller, like a gym env
    f = env.reset()
    assert f.shape == (210, 160, 3) and f.dtype == np.uint8
    d = hash32(3, 1, 0)
    assert (env.ball_x, env.ball_y, env.vx, env.vy) == (8 + d % 56, 40, 1 if (d >> 8) & 1 else -1, -1) and env.draws == 1
    assert (env.paddle_x, env.lives_left, env.bricks_left, env.ep_steps) == (32, 5, 108, 0) and env.rows == [FULL_ROW] * 6
    assert env.render().shape == (210, 160, 3)
    env.seed(4)
    env.reset()
    assert env.ball_x == 8 + hash32(4, 1, 1) % 56


def test_the_constants_are_the_documented_ones():
    assert (breakout.W, breakout.H) == (72, 80) and breakout.N_ACTIONS == 4
    assert (breakout.BRICK_ROWS, breakout.BRICK_COLS, breakout.BRICK_W, breakout.BRICK_H, breakout.BRICK_TOP) == (6, 18, 4, 3, 11)
    assert ROW_LEVEL == (200, 198, 180, 162, 72, 66) and ROW_POINTS == (7, 7, 4, 4, 1, 1)
    assert [rgb[0] for rgb in breakout.ROW_RGB] == list(ROW_LEVEL)
    assert HIT_VX == (-2, -2, -1, -1, 0, 1, 1, 2, 2)
    assert (breakout.PADDLE_W, breakout.PADDLE_H, breakout.PADDLE_Y, breakout.PADDLE_MAX_X, breakout.PADDLE_SPEED) == (8, 2, 77, 64, 3)
    assert (breakout.BALL, breakout.BALL_MAX_X, breakout.LOST_Y, breakout.STATE_WORDS) == (2, 70, 78, 24)


# ---------------------------------------------------------------- the rules, on hand-built positions
@pytest.mark.parametrize("x, vx, want_x, want_vx", [(1, -2, 1, 2), (0, -1, 1, 1), (1, -1, 0, -1), (0, -2, 2, 2),
                                                    (69, 2, 69, -2), (70, 1, 69, -1), (69, 1, 70, 1), (70, 2, 68, -2)])
def test_both_side_walls(x, vx, want_x, want_vx):
    env = position(ball=(x, 50), vel=(vx, 1))
    _, rew, done, _ = env.step(NOOP)
    assert (rew, done) == (0.0, False)
    assert (env.ball_x, env.ball_y, env.vx, env.vy) == (want_x, 51, want_vx, 1)
    assert events(env, side_wall=1 if want_vx != vx else 0)


@pytest.mark.parametrize("y, vy, want_y, want_vy", [(1, -2, 1, 2), (0, -1, 1, 1), (1, -1, 0, -1), (0, -2, 2, 2), (2, -2, 0, -2)])
def test_the_ceiling(y, vy, want_y, want_vy):
    env = position(ball=(20, y), vel=(1, vy))
    _, rew, done, _ = env.step(NOOP)
    assert (rew, done) == (0.0, False)
    assert (env.ball_x, env.ball_y, env.vx, env.vy) == (21, want_y, 1, want_vy)
    assert events(env, ceiling=1 if want_vy != vy else 0)


def test_a_brick_hit_from_below():
    env = position(ball=(10, 30), vel=(1, -1))
    assert env.step(NOOP)[1:3] == (0.0, False) and (env.ball_x, env.ball_y, env.vy) == (11, 29, -1)      # ly = 29: under the wall
    _, rew, done, _ = env.step(NOOP)              # leading corner (13, 28): brick row 5, column 3
    assert (rew, done) == (1.0, False)
    assert (env.ball_x, env.ball_y, env.vx, env.vy) == (12, 29, 1, 1), "y goes back to the old y, x keeps the new value"
    assert env.rows == [FULL_ROW] * 5 + [FULL_ROW & ~(1 << 3)] and env.bricks_left == 107
    assert events(env, brick=1)
    assert env.step(NOOP)[1] == 0.0 and env.ball_y == 30 and env.bricks_left == 107


def test_a_brick_hit_from_above_with_the_ball_behind_the_wall():
    env = position(ball=(10, 8), vel=(1, 1))
    assert env.step(NOOP)[1] == 0.0 and (env.ball_x, env.ball_y) == (11, 9)          # leading corner row 10: above the wall
    _, rew, done, _ = env.step(NOOP)              # leading corner (13, 11): brick row 0, column 3
    assert (rew, done) == (7.0, False)
    assert (env.ball_x, env.ball_y, env.vx, env.vy) == (12, 9, 1, -2), "bounced upwards, sped up by a top row"
    assert env.rows == [FULL_ROW & ~(1 << 3)] + [FULL_ROW] * 5
    assert events(env, brick=1, speed_up=1)


def test_the_leading_corner_follows_the_velocity():
    # moving left and up the corner is the ball's own top-left pixel: (7, 28) is brick column 1, not column 2
    env = position(ball=(8, 29), vel=(-1, -1))
    assert env.step(NOOP)[1] == 1.0 and env.rows[5] == FULL_ROW & ~(1 << 1)
    # after a side-wall bounce the corner is taken with the new vx: x = 1, vx = +2 -> lx = 2, column 0
    env = position(ball=(1, 29), vel=(-2, -1))
    assert env.step(NOOP)[1] == 1.0 and env.rows[5] == FULL_ROW & ~1 and env.vx == 2
    assert events(env, side_wall=1, brick=1)


@pytest.mark.parametrize("r", range(6))
@pytest.mark.parametrize("vy0", [-1, -2])
def test_every_rows_points_and_the_speed_up_of_the_upper_three(r, vy0):
    col = 5
    rows = [FULL_ROW if k <= r else FULL_ROW & ~(1 << col) for k in range(6)]      # column 5 is open below row r
    y0 = 11 + 3 * r + 3                           # the ball's top edge right under brick row r
    env = position(ball=(4 * col + 1, y0), vel=(1, vy0), rows=rows)
    _, rew, done, _ = env.step(NOOP)
    assert (rew, done) == (float(ROW_POINTS[r]), False)
    assert env.rows[r] == FULL_ROW & ~(1 << col) and env.ball_y == y0
    assert env.vy == (2 if r < 3 else -vy0), "rows 0..2 set |vy| = 2, rows 3..5 only flip the sign"
    assert events(env, brick=1, speed_up=1 if (r < 3 and vy0 == -1) else 0)


def test_at_most_one_brick_dies_per_step():
    env = position(ball=(2, 31), vel=(2, -2))     # leading corner (5, 29)... then (7, 27): one brick per step
    n0 = env.bricks_left
    env.step(NOOP)
    assert env.bricks_left == n0
    env.step(NOOP)
    assert env.bricks_left == n0 - 1
    env.step(NOOP)                                # moving down and away now
    assert env.bricks_left == n0 - 1


@pytest.mark.parametrize("off", range(9))
@pytest.mark.parametrize("vy", [1, 2])
@pytest.mark.parametrize("vx", [1, -1])
def test_paddle_hit_with_each_table_entry(off, vy, vx):
    px = 30
    x = px - 1 + off                              # off = ball x + 1 - paddle x
    env = position(ball=(x - vx, 76 - vy), vel=(vx, vy), px=px)
    _, rew, done, _ = env.step(NOOP)
    assert (rew, done) == (0.0, False)
    assert (env.ball_x, env.ball_y) == (x, 75), "the ball rests on the paddle"
    assert env.vy == -vy, "|vy| survives the paddle: only a serve resets a speed-up"
    assert env.vx == (HIT_VX[off] if off != 4 else vx), "the centre keeps the direction, |vx| = 1"
    assert env.vx != 0 and events(env, paddle_hit=1)


@pytest.mark.parametrize("x", [28, 38])
def test_a_ball_beside_the_paddle_is_not_hit(x):
    env = position(ball=(x, 75), vel=(0, 1), px=30)
    env.vx = 1
    env.ball_x = x - 1
    env.step(NOOP)
    assert events(env) and (env.ball_x, env.ball_y, env.vy) == (x, 76, 1)


def test_the_paddle_moves_before_the_ball_is_judged():
    # the ball comes down two columns right of the paddle's reach; moving right (3 pixels) in the same step catches it
    env = position(ball=(39, 75), vel=(1, 1), px=30)
    env.step(NOOP)
    assert events(env) and env.ball_y == 76
    env = position(ball=(39, 75), vel=(1, 1), px=30)
    env.step(RIGHT)
    assert events(env, paddle_hit=1) and env.paddle_x == 33 and (env.ball_x, env.ball_y, env.vx, env.vy) == (40, 75, 2, -1)


def test_a_ball_not_caught_when_it_reaches_the_paddles_row_is_never_caught():
    env = position(ball=(50, 75), vel=(1, 1), px=0, seed=5, env_id=2)
    env.step(NOOP)                                # y = 76: reaches row 77 beside the paddle
    env.paddle_x = 48                             # the paddle under it now
    out = []
    for _ in range(3):
        d0 = env.draws
        out.append(env.step(NOOP)[1:3])
        if env.events["life_lost"]:
            break
    assert out == [(0.0, False)] * 3 and events(env, life_lost=1), "y: 77, 78, then 79 > 78"
    d = hash32(5, 2, d0)
    assert env.lives_left == 4 and env.draws == d0 + 1
    assert (env.ball_x, env.ball_y, env.vx, env.vy) == (8 + d % 56, 40, 1 if (d >> 8) & 1 else -1, -1)
    assert env.paddle_x == 48 and env.bricks_left == 108, "a serve moves the ball only"


def test_the_serve_resets_a_speed_up():
    env = position(ball=(50, 77), vel=(1, 2), px=0)
    env.step(NOOP)
    assert events(env, life_lost=1) and env.vy == -1 and abs(env.vx) == 1


def test_serves_go_both_ways_from_every_part_of_the_field():
    xs, ways = set(), set()
    for j in range(200):
        env = BreakoutEnv(seed=1, env_id=j)
        env.reset()
        xs.add(env.ball_x)
        ways.add(env.vx)
        assert env.ball_y == 40 and env.vy == -1
    assert ways == {1, -1} and min(xs) >= 8 and max(xs) <= 63 and len(xs) > 40


def test_paddle_moves_three_pixels_and_clamps_at_both_edges():
    env = position(px=4)
    xs = []
    for a in (LEFT, LEFT, LEFT, RIGHT, NOOP, FIRE, 4 + LEFT, -2, -1):      # actions are taken mod 4: 7 is left, -2 right, -1 left
        env.ball_x, env.ball_y, env.vx, env.vy = 30, 50, 1, 1               # keep the ball in mid field
        env.step(a)
        xs.append(env.paddle_x)
    assert xs == [1, 0, 0, 3, 3, 3, 0, 3, 0]
    env = position(px=60)
    for a, want in ((RIGHT, 63), (RIGHT, 64), (RIGHT, 64), (LEFT, 61)):
        env.ball_x, env.ball_y, env.vx, env.vy = 30, 50, 1, 1
        env.step(a)
        assert env.paddle_x == want


def test_the_last_life_lost_is_a_real_done():
    env = position(ball=(50, 78), vel=(1, 1), px=0, lives_left=1, lives=3)
    d0 = env.draws
    _, rew, done, _ = env.step(NOOP)
    assert (rew, done) == (0.0, True) and env.lives_left == 0 and env.draws == d0      # no serve: the caller resets
    assert events(env, life_lost=1, episode_end=1)
    with pytest.raises(RuntimeError):
        env.step(NOOP)
    env.reset()
    assert (env.lives_left, env.bricks_left, env.ep_steps, env.paddle_x) == (3, 108, 0, 32) and env.draws == d0 + 1
    env = position(ball=(50, 78), vel=(1, 1), px=0, lives_left=2)
    assert env.step(NOOP)[2] is False and env.lives_left == 1


def test_the_last_brick_is_a_real_done():
    rows = [0, 0, 0, 1 << 7, 0, 0]
    env = position(ball=(29, 23), vel=(1, -1), rows=rows)      # leading corner (30, 22): row 3, column 7
    assert env.bricks_left == 1
    _, rew, done, _ = env.step(NOOP)
    assert (rew, done) == (4.0, True) and env.bricks_left == 0 and env.rows == [0] * 6
    assert events(env, brick=1, cleared=1, episode_end=1)
    env.reset()
    assert env.bricks_left == 108 and env.rows == [FULL_ROW] * 6


def test_max_episode_steps_is_a_real_done():
    env = position(max_episode_steps=5)
    out = [env.step(NOOP)[1:3] for _ in range(5)]
    assert out == [(0.0, False)] * 4 + [(0.0, True)]
    env.reset()
    assert env.ep_steps == 0 and env.steps == 5
    assert [env.step(NOOP)[2] for _ in range(5)] == [False] * 4 + [True]


def test_fire_equals_noop():
    world = dict(seed=6, env_id=1, lives=1, max_episode_steps=150)
    a, b = BreakoutEnv(**world), BreakoutEnv(**world)
    a.reset()
    b.reset()
    n_done = 0
    for t in range(400):
        move = tracking_action(a, 6, 1, t)
        ra, rb = a.advance(move if move >= 2 else NOOP), b.advance(move if move >= 2 else FIRE)
        assert ra == rb and np.array_equal(a.state_words(), b.state_words()), t
        if ra[1]:
            n_done += 1
            a.new_episode()
            b.new_episode()
    assert n_done >= 1 and a.events["paddle_hit"] >= 1 and a.events == b.events


# ---------------------------------------------------------------- frames
def expected_frame(env):
    want = np.zeros((80, 72), dtype=np.uint8)
    for r in range(6):
        for c in range(18):
            if (env.rows[r] >> c) & 1:
                want[11 + 3 * r:14 + 3 * r, 4 * c:4 * c + 4] = ROW_LEVEL[r]
    want[77:79, env.paddle_x:env.paddle_x + 8] = 200
    want[env.ball_y:env.ball_y + 2, env.ball_x:env.ball_x + 2] = 200
    return want


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_breakout_prep_of_the_raw_frame_is_the_prepped_frame(seed):
    env = BreakoutEnv(seed=seed, env_id=seed + 1, lives=2)
    raw = env.reset()
    levels = set()
    for t in range(200):
        y = preprocessing.breakout_prep(raw)
        assert y.shape == (1, 80, 72) and y.dtype == np.uint8
        np.testing.assert_array_equal(y, env.prepped())
        np.testing.assert_array_equal(y[0], expected_frame(env))
        levels |= set(np.unique(y).tolist())
        raw, rew, done, _ = env.step(tracking_action(env, seed, 0, t))
        if done:
            raw = env.reset()
    assert levels - {0} == set(ROW_LEVEL), "six grey levels besides the background"
    assert len(levels - {0}) >= 4 and env.events["brick"] > 0 and env.events["paddle_hit"] > 0


def test_raw_frame_layout():
    env = position(ball=(20, 5), px=64, rows=[1, 0, 0, 0, 0, 1 << 17])
    raw = env.render_rgb()
    assert raw.shape == (210, 160, 3) and raw.dtype == np.uint8
    assert (raw[:17] == 0).all() and (raw[195:] == 0).all(), "black above the walls and below the field"
    assert (raw[17:35] == 142).all() and (raw[17:195, :8] == 142).all() and (raw[17:195, 152:] == 142).all()
    field = raw[35:195, 8:152]
    assert (field[10:14, 40:44] == np.array(breakout.OBJECT_RGB)).all()                      # the ball, 2 x scale
    assert (field[154:158, 128:144] == np.array(breakout.OBJECT_RGB)).all()                  # the paddle at the right edge
    assert (field[22:28, 0:8] == np.array(breakout.ROW_RGB[0])).all() and (field[52:58, 136:144] == np.array(breakout.ROW_RGB[5])).all()
    assert (field.reshape(-1, 3).any(axis=1)).sum() == 4 * (4 + 16 + 12 + 12)


# ---------------------------------------------------------------- randomness, state words
def play(env, n, tape_seed=0):
    env.reset()
    out, rews = [env.prepped().copy()], []
    for t in range(n):
        obs, rew, done, _ = env.step(tracking_action(env, tape_seed, 0, t))
        if done:
            env.reset()
        out.append(env.prepped().copy())
        rews.append((rew, done))
    return out, rews


def test_same_seed_and_env_id_give_the_same_trajectory():
    a, ra = play(BreakoutEnv(seed=21, env_id=3, max_episode_steps=150), 400)
    b, rb = play(BreakoutEnv(seed=21, env_id=3, max_episode_steps=150), 400)
    assert ra == rb and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert any(r for r, _ in ra) and any(d for _, d in ra)


def test_different_env_ids_and_seeds_get_different_worlds():
    a, ra = play(BreakoutEnv(seed=21, env_id=0), 200)
    b, rb = play(BreakoutEnv(seed=21, env_id=1), 200)
    c, rc = play(BreakoutEnv(seed=22, env_id=0), 200)
    assert not all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not all(np.array_equal(x, y) for x, y in zip(a, c))


def test_state_words_carry_a_position_from_one_twin_to_another():
    a = BreakoutEnv(seed=8, env_id=5, lives=2)
    a.reset()
    for t in range(150):
        if a.advance(tracking_action(a, 8, 0, t))[1]:
            a.new_episode()
    w = a.state_words()
    assert w.shape == (24,) and w.dtype == np.int32 and (w[17:] == 0).all()
    assert list(w[:11]) == [a.paddle_x, a.ball_x, a.ball_y, a.vx, a.vy, a.lives_left, a.bricks_left, a.draws, a.steps,
                            a.ep_steps, a.ep_rew]
    assert list(w[11:17]) == a.rows and sum(bin(m).count("1") for m in a.rows) == a.bricks_left < 108
    b = BreakoutEnv(seed=8, env_id=5, lives=2)
    b.load_state_words(w)
    for t in range(300):
        move = tracking_action(a, 9, 0, t)
        ra, rb = a.advance(move), b.advance(move)
        assert ra == rb and np.array_equal(a.state_words(), b.state_words()) and np.array_equal(a.prepped(), b.prepped())
        if ra[1]:
            a.new_episode()
            b.new_episode()
    assert a.events["brick"] >= 1 and a.events["paddle_hit"] >= 1


# ---------------------------------------------------------------- bounds
def test_world_from_hyps_bounds():
    assert world_from_hyps({}) == (5, 10000)
    assert world_from_hyps(dict(lives=1, max_episode_steps=1)) == (1, 1)
    assert world_from_hyps(dict(lives=None, max_episode_steps=1 << 24)) == (5, 1 << 24)
    for bad in (dict(lives=0), dict(lives=6), dict(lives=-1), dict(max_episode_steps=0), dict(max_episode_steps=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            world_from_hyps(bad)
        with pytest.raises(ValueError):
            BreakoutEnv(**bad)


# ---------------------------------------------------------------- behind the host pools
def test_breakout_env_behind_sequential_environment_and_host_pool():
    mk = lambda j: SequentialEnvironment("Breakout-host", preprocessing.breakout_prep, env_fn=BreakoutFactory(seed=2, env_id=j))
    env = mk(0)
    assert env.is_discrete and env.n == 4 and env.raw_shape == (210, 160, 3)
    obs = env.reset()
    assert obs.shape == (1, 80, 72) and obs.dtype == np.uint8 and set(np.unique(obs)) == {0} | set(ROW_LEVEL)
    pool = HostEnvPool([mk(j) for j in range(3)], frame_shape=(1, 80, 72))
    assert len(pool) == 3 and pool.reset(1).shape == (1, 80, 72)
    obs, rew, done = pool.step(1, RIGHT)
    assert obs.shape == (1, 80, 72) and rew == 0.0 and done is False
    f = pickle.loads(pickle.dumps(BreakoutFactory(env_id=4, seed=2, lives=3)))      # travels to the env workers
    assert f().env_id == 4 and f().lives == 3


def test_breakout_env_behind_the_process_pool_with_the_uint8_transport():
    """what train(env_type="Breakout-host") builds without env_pool="serial": worker processes stepping BreakoutEnvs through
    breakout_prep, the grey frames crossing the pinned region one byte per pixel, done = the real done"""
    from a2c_amd.hostpool import FRAME_U8, ProcessEnvPool
    B, K = 3, 60
    world = dict(seed=4, lives=1, max_episode_steps=40)
    kws = [dict(env_type="Breakout-host", preprocessor=preprocessing.breakout_prep, seed=4,
                env_fn=BreakoutFactory(env_id=j, **world)) for j in range(B)]
    pool = ProcessEnvPool(SequentialEnvironment, B, env_kwargs=kws, n_workers=2, pong=False, register=False, frame_bits=False)
    refs = [SequentialEnvironment(**kw) for kw in kws]
    try:
        pool.start()
        pool.set_phase(1)
        h = pool.header
        assert h.frame_dtype == FRAME_U8 and h.frame_bytes == 5760 and h.frame_elems == 5760
        pool.wait_frames(0)
        for j in range(B):
            assert np.array_equal(pool.frames_view()[j].reshape(1, 80, 72), refs[j].reset())
        rew, done = np.zeros(B, np.float32), np.zeros(B, np.float32)
        n_done, levels = 0, set()
        for k in range(K):
            acts = np.array([hash32(4, 50 + j, k) % 4 for j in range(B)], np.int64)
            pool.post_actions(acts, seq=k)
            pool.wait_frames(k + 1)
            pool.unpack(rew, done)
            fr = pool.frames_view()
            for j in range(B):
                o, r, d, _ = refs[j].step(int(acts[j]))
                if d:
                    o = refs[j].reset()
                assert np.array_equal(fr[j].reshape(1, 80, 72), o), (k, j)
                assert rew[j] == np.float32(r) and done[j] == float(d), (k, j)
                n_done += d
            levels |= set(np.unique(fr).tolist())
        assert n_done >= B and levels == {0} | set(ROW_LEVEL)
    finally:
        pool.close()
