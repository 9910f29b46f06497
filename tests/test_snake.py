"""Snake on the host (no GPU needed): ``snake_prep`` against vectors recorded from the reference's own function
(tests/golden/g11_snake_prep.npz, made by tests/golden/make_golden_snake.py), the rules of ``a2c_amd.snake.SnakeEnv`` on
hand-built positions, determinism of the counter-based draws, and the env behind the host pools.  The device worlds are
compared with this host twin, value for value, in test_gpu_snake.py."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from a2c_amd import preprocessing
from a2c_amd.runner import HostEnvPool, SequentialEnvironment
from a2c_amd.snake import BODY, FOOD, HEAD, SPACE, SnakeEnv, SnakeFactory, hash32, world_from_hyps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference/a2c"
UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3


def position(G=6, u=2, n_foods=2, body=((2, 2), (2, 1), (2, 0)), foods=((0, 0), (5, 5)), **kw):
    """an env in a hand-built position: body[0] is the head, body[-1] the tail"""
    env = SnakeEnv(grid_size=G, unit_size=u, n_foods=n_foods, **kw)
    env.reset()
    env.cells[:] = 0
    L = len(body)
    for i, rc in enumerate(body):
        env.cells[rc] = L - i
    for rc in foods:
        env.cells[rc] = -1
    env.head, env.length, env.over = tuple(body[0]), L, False
    return env


def cell_colours(env, frame):
    u = env.u
    assert frame.shape == (env.G * u, env.G * u, 3) and frame.dtype == np.uint8
    blocks = frame.reshape(env.G, u, env.G, u, 3)
    assert (blocks == blocks[:, :1, :, :1]).all(), "a cell is one colour"
    return blocks[:, 0, :, 0]


# ---------------------------------------------------------------- snake_prep
def test_snake_prep_matches_the_reference_vectors(golden):
    g = golden["g11_snake_prep"]
    names = sorted(k[:-4] for k in g.files if k.endswith("_raw"))
    assert len(names) >= 20
    for n in names:
        y = preprocessing.snake_prep(g[n + "_raw"])
        assert y.dtype == np.float32 and y.shape == g[n + "_prep"].shape
        np.testing.assert_array_equal(y, g[n + "_prep"], err_msg=n)


def test_the_recorded_raw_frames_are_what_snake_env_produces(golden):
    import make_golden_snake as M
    g = golden["g11_snake_prep"]
    for n, pic in M.raw_frames().items():
        np.testing.assert_array_equal(pic, g[n + "_raw"], err_msg=n)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is only in the build container")
def test_g11_regenerates_bit_identically(tmp_path):
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import make_golden_snake as M; "
            "np.savez(%r, **M.build())" % (os.path.join(ROOT, "tests", "golden"), str(tmp_path / "g11.npz")))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=str(tmp_path), capture_output=True)
    new = np.load(tmp_path / "g11.npz")
    old = np.load(os.path.join(ROOT, "tests", "golden", "g11_snake_prep.npz"))
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)


# ---------------------------------------------------------------- the rules, on hand-built positions
def test_surface_and_reset():
    env = SnakeEnv(seed=3, env_id=1)
    assert env.action_space.n == 4
    f = env.reset()
    assert f.shape == (60, 60, 3) and f.dtype == np.uint8
    c = env.cells
    assert env.length == 3 and sorted(c[c > 0]) == [1, 2, 3] and (c < 0).sum() == 2 and c[env.head] == 3
    # the three body cells lie in one line, head first
    (r3, c3), (r2, c2), (r1, c1) = (tuple(np.argwhere(c == v)[0]) for v in (3, 2, 1))
    assert (r3 - r2, c3 - c2) == (r2 - r1, c2 - c1) and abs(r3 - r2) + abs(c3 - c2) == 1
    with pytest.raises(ValueError):
        SnakeEnv(grid_size=15, unit_size=4, n_foods=15 * 15 - 3)
    with pytest.raises(ValueError):
        SnakeEnv(grid_size=3)
    with pytest.raises(ValueError):
        SnakeEnv(grid_size=5, unit_size=1)          # 25 pixels: not a multiple of 4
    assert world_from_hyps(dict(grid_size=[21, 21], unit_size=4, n_foods=3)) == (21, 4, 3)
    assert world_from_hyps({}) == (15, 4, 2)


def test_frame_colours_per_cell():
    env = position()
    col = cell_colours(env, env.render_rgb())
    assert tuple(col[2, 2]) == HEAD == (255, 0, 0)
    assert tuple(col[2, 1]) == BODY == (1, 0, 0) and tuple(col[2, 0]) == BODY
    assert tuple(col[0, 0]) == FOOD == (0, 0, 255) and tuple(col[5, 5]) == FOOD
    assert tuple(col[3, 3]) == SPACE == (0, 255, 0)
    assert (col == np.array(SPACE)).all(-1).sum() == 36 - 5
    prep = preprocessing.snake_prep(env.render_rgb())[0][::2, ::2]
    assert prep[2, 2] == np.float32(1.5) and prep[2, 1] == 1 and prep[0, 0] == np.float32(.33) and prep[3, 3] == 0


def test_plain_move_vacates_the_tail():
    env = position()
    _, rew, done, _ = env.step(RIGHT)
    assert (rew, done) == (0.0, False) and env.head == (2, 3) and env.length == 3
    assert env.cells[2, 3] == 3 and env.cells[2, 2] == 2 and env.cells[2, 1] == 1 and env.cells[2, 0] == 0
    _, rew, done, _ = env.step(UP)
    assert (rew, done) == (0.0, False) and env.head == (1, 3) and env.cells[2, 1] == 0


@pytest.mark.parametrize("body, action", [(((0, 2), (1, 2), (2, 2)), UP), (((2, 5), (2, 4), (2, 3)), RIGHT),
                                          (((5, 2), (4, 2), (3, 2)), DOWN), (((2, 0), (2, 1), (2, 2)), LEFT)])
def test_wall_death(body, action):
    env = position(body=body, foods=((0, 0), (5, 5)))
    before = env.cells.copy()
    _, rew, done, _ = env.step(action)
    assert (rew, done) == (-1.0, True)
    np.testing.assert_array_equal(env.cells, before)
    with pytest.raises(RuntimeError):
        env.step(action)


def test_neck_death():
    env = position()                              # head (2,2), neck (2,1)
    _, rew, done, _ = env.step(LEFT)
    assert (rew, done) == (-1.0, True)


def test_tail_cell_death():
    # a 2x2 loop of length 4: the head moves onto the cell the tail still holds -- vacated after the move, not before
    env = position(body=((2, 2), (2, 3), (3, 3), (3, 2)))
    assert env.cells[3, 2] == 1
    _, rew, done, _ = env.step(DOWN)
    assert (rew, done) == (-1.0, True)
    # with one more free step in between the same cell is free
    env = position(body=((2, 2), (2, 3), (3, 3)))
    _, rew, done, _ = env.step(DOWN)
    assert (rew, done) == (0.0, False) and env.head == (3, 2)


def test_food_and_growth():
    env = position(foods=((2, 3), (5, 5)))
    d0 = env.draws
    _, rew, done, _ = env.step(RIGHT)
    assert (rew, done) == (1.0, False) and env.length == 4 and env.head == (2, 3)
    c = env.cells
    assert c[2, 3] == 4 and c[2, 2] == 3 and c[2, 1] == 2 and c[2, 0] == 1       # nothing vacated
    assert (c < 0).sum() == 2 and c[5, 5] == -1 and env.draws == d0 + 1
    # the new food is the k-th free cell in row-major order, k = draw mod n_free
    n_free = 36 - 4 - 1
    k = hash32(env.seed_, env.env_id, d0) % n_free
    was_free = [(r, q) for r in range(6) for q in range(6) if (r, q) not in ((2, 3), (2, 2), (2, 1), (2, 0), (5, 5))]
    assert c[was_free[k]] == -1
    _, rew, done, _ = env.step(RIGHT)             # the grown snake keeps its length
    assert rew == 0.0 and (env.cells > 0).sum() == 4


def test_full_grid_ends_the_episode():
    G = 4
    snake_path = [(r, q if r % 2 == 0 else G - 1 - q) for r in range(G) for q in range(G)]      # boustrophedon, 16 cells
    body = tuple(reversed(snake_path[:14]))       # head at path[13], two cells left: both foods
    env = position(G=G, u=2, n_foods=2, body=body, foods=(snake_path[14], snake_path[15]))
    assert (env.cells == 0).sum() == 0
    step_to = lambda a, b: {(-1, 0): UP, (0, 1): RIGHT, (1, 0): DOWN, (0, -1): LEFT}[(b[0] - a[0], b[1] - a[1])]
    _, rew, done, _ = env.step(step_to(snake_path[13], snake_path[14]))
    assert (rew, done) == (1.0, True) and env.length == 15      # no free cell for a new food: the grid is full


def test_reset_after_done_starts_a_new_episode():
    env = position(body=((0, 2), (1, 2), (2, 2)), seed=4, env_id=9)
    d0 = env.draws
    env.step(UP)
    f = env.reset()
    assert env.length == 3 and not env.over and (env.cells < 0).sum() == 2 and env.draws == d0 + 2 + 2
    np.testing.assert_array_equal(f, env.render_rgb())
    env.step(UP)                                  # stepping is legal again


# ---------------------------------------------------------------- randomness
def test_hash32_is_the_documented_finaliser():
    def fin(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = x * 0x7FEB352D & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846CA68B & 0xFFFFFFFF
        return x ^ (x >> 16)
    for seed, e, i in ((0, 0, 0), (1, 2, 3), (2 ** 32 - 1, 70000, 2 ** 31)):
        assert hash32(seed, e, i) == fin(fin(fin(seed + 0x9E3779B9) ^ e) ^ i)
    assert len({hash32(5, e, i) for e in range(64) for i in range(64)}) == 4096


def play(env, n, tape_seed=0):
    out = [env.reset().copy()]
    rews = []
    for t in range(n):
        obs, rew, done, _ = env.step(hash32(tape_seed, 0, t) & 3)
        if done:
            obs = env.reset()
        out.append(obs.copy())
        rews.append((rew, done))
    return out, rews


def test_same_seed_and_env_id_give_the_same_trajectory():
    a, ra = play(SnakeEnv(seed=21, env_id=3), 200)
    b, rb = play(SnakeEnv(seed=21, env_id=3), 200)
    assert ra == rb and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert any(d for _, d in ra)


def test_different_env_ids_get_different_worlds():
    foods = set()
    for e in range(8):
        env = SnakeEnv(seed=21, env_id=e)
        env.reset()
        foods.add(tuple(map(tuple, np.argwhere(env.cells < 0))))
    assert len(foods) >= 7
    a, _ = play(SnakeEnv(seed=21, env_id=0), 50)
    b, _ = play(SnakeEnv(seed=22, env_id=0), 50)
    assert not all(np.array_equal(x, y) for x, y in zip(a, b))


def test_free_cell_pick_never_lands_on_an_occupied_cell():
    """10^4 random steps of a small, crowded world: after every step the grid holds exactly n_foods foods, `length` body
    cells with lifetimes 1..length, and nothing else (a pick on an occupied cell would lose a food or a body cell)"""
    env = SnakeEnv(seed=8, env_id=0, grid_size=5, unit_size=2, n_foods=6)
    env.reset()
    foods_eaten = deaths = 0
    for t in range(10 ** 4):
        _, rew, done, _ = env.step(hash32(77, 1, t) & 3)
        foods_eaten += rew > 0
        deaths += done
        if done:
            env.reset()
        c = env.cells
        assert (c < 0).sum() == env.n_foods and (c >= -1).all()
        assert sorted(c[c > 0]) == list(range(1, env.length + 1)) and c[env.head] == env.length
    assert foods_eaten > 100 and deaths > 100


# ---------------------------------------------------------------- behind the host pools
def test_snake_env_behind_sequential_environment_and_host_pool():
    mk = lambda j: SequentialEnvironment("Snake-host", preprocessing.snake_prep,
                                         env_fn=SnakeFactory(seed=2, env_id=j, grid_size=6, unit_size=2, n_foods=2))
    env = mk(0)
    assert env.is_discrete and env.n == 4 and env.raw_shape == (12, 12, 3)
    obs = env.reset()
    assert obs.shape == (1, 12, 12) and obs.dtype == np.float32
    assert set(np.unique(obs)) == {np.float32(0), np.float32(.33), np.float32(1), np.float32(1.5)}
    pool = HostEnvPool([mk(j) for j in range(3)], frame_shape=(1, 12, 12))
    assert len(pool) == 3 and pool.reset(1).shape == (1, 12, 12)
    obs, rew, done = pool.step(1, 0)
    assert obs.shape == (1, 12, 12) and rew in (-1.0, 0.0, 1.0) and isinstance(done, bool)
    f = pickle.loads(pickle.dumps(SnakeFactory(seed=2, env_id=4)))      # travels to the env worker processes
    assert f().env_id == 4
