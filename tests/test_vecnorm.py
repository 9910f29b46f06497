"""CPU: ``a2c_amd.vecnorm.RunningNorm``, the host twin of a2c_vecnorm_step, against the textbook formulas; the reward rule;
clipping; a constant feature; ``state_dict``; the frozen mode; what ``train()`` and the Runner refuse without a GPU."""
import numpy as np
import pytest

from a2c_amd.vecnorm import COUNT0, RunningNorm, lane_sum


def test_running_moments_equal_the_textbook_on_the_history():
    """50 batches of mixed sizes: running mean / var against np.mean / np.var (float64) of everything seen.  The two differ in
    summation order only, so 1e-12 relative bounds rounding: a float64 sum of n <= 2e4 terms carries at most n * 2^-53 ~ 2e-12
    relative error in the worst case and ~ sqrt(n) * 2^-53 ~ 2e-14 in the mean, and the combination rule adds a few roundings
    per batch.  Baselines' start is 1e-4 phantom samples of mean 0 and variance 1, which np.mean / np.var of the history do not
    hold: the comparison is made once from a count of 0, the history alone, and once from the real start with the phantom
    samples combined in exactly."""
    g = np.random.default_rng(0)
    L, P = 6, 1200
    rn, bare = RunningNorm(L, P, 0.99), RunningNorm(L, P, 0.99)
    bare.obs_count = np.float64(0.0)           # no phantom samples: the history and nothing else
    scale, shift = 10.0 ** g.uniform(-2, 3, L), g.uniform(-50, 50, L)
    hist = []
    for k in range(50):
        B = int(g.choice([1, 2, 7, 64, 255, 256, 257, 700, 1200]))
        x = (g.standard_normal((B, L)) * scale + shift).astype(np.float32)
        hist.append(x.astype(np.float64))
        rn.step(x, None, None, 0)
        bare.step(x, None, None, 0)
    h = np.concatenate(hist)
    n = h.shape[0]
    assert bare.obs_count == n and n > 5000
    np.testing.assert_allclose(bare.obs_mean, h.mean(0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(bare.obs_var, h.var(0), rtol=1e-12, atol=0)
    # from baselines' start the 1e-4 phantom samples (mean 0, var 1) are in as well: the same history, combined with them
    assert rn.obs_count == pytest.approx(COUNT0 + n, rel=1e-15)
    c0, tot = COUNT0, COUNT0 + n
    mean = h.mean(0) * n / tot
    var = (c0 * 1.0 + n * h.var(0) + h.mean(0) ** 2 * c0 * n / tot) / tot
    np.testing.assert_allclose(rn.obs_mean, mean, rtol=1e-12, atol=0)
    np.testing.assert_allclose(rn.obs_var, var, rtol=1e-12, atol=0)


def test_lane_sum_is_the_256_lane_order():
    """lane i adds rows i, i + 256, ... in order; then strides 128 .. 1"""
    g = np.random.default_rng(1)
    v = g.standard_normal(700) * 10.0 ** g.uniform(-8, 8, 700)
    part = [0.0] * 256
    for i, x in enumerate(v):
        part[i % 256] = part[i % 256] + x
    s = 128
    while s:
        for i in range(s):
            part[i] = part[i] + part[i + s]
        s //= 2
    assert lane_sum(v) == part[0]
    assert lane_sum(np.ones((3, 2))).tolist() == [3.0, 3.0]


def test_reward_rule_on_a_hand_made_sequence():
    """ret = ret * gamma + r; the return's moments take ret; r / sqrt(var + eps); THEN ret = 0 where done"""
    gamma, eps = 0.5, 1e-8
    rn = RunningNorm(1, 2, gamma, eps=eps, clip_rew=1e9)
    rews = np.array([[1.0, 2.0], [3.0, -1.0], [0.5, 4.0], [2.0, 2.0]], dtype=np.float32)
    dones = np.array([[0, 0], [1, 0], [0, 1], [0, 0]], dtype=np.float32)
    ret, seen = np.zeros(2), []
    for r, d in zip(rews, dones):
        ret = ret * gamma + r
        seen.append(ret.copy())
        _, out = rn.step(None, r, d, 0)
        # the moments of every ret value so far (and the 1e-4 phantom samples of mean 0, var 1)
        h = np.concatenate(seen)
        n, tot = len(h), COUNT0 + len(h)
        var = (COUNT0 + n * h.var() + h.mean() ** 2 * COUNT0 * n / tot) / tot
        np.testing.assert_allclose(rn.ret_var, var, rtol=1e-12)
        np.testing.assert_allclose(out, (r / np.sqrt(var + eps)).astype(np.float32), rtol=1e-6)
        ret = np.where(d != 0, 0.0, ret)
        assert rn.ret.tolist() == ret.tolist()
    # step 1 closed env 0 with ret = 1 * .5 + 3 = 3.5 INSIDE the moments: zeroing before the division would have fed 0
    assert seen[1][0] == 3.5 and seen[2][0] == 0.5 and seen[3][1] == 2.0
    assert rn.obs_count == COUNT0 and rn.ret_count == COUNT0 + 8


def test_sub_ranges_keep_their_own_accumulators():
    rn = RunningNorm(2, 6, 0.9)
    rn.step(None, np.ones(2, np.float32), np.zeros(2), 3)
    assert rn.ret.tolist() == [0, 0, 0, 1, 1, 0]
    for env0, B in ((-1, 2), (5, 2), (0, 7)):
        with pytest.raises(ValueError):
            rn.step(None, np.ones(B, np.float32), np.zeros(B), env0)
    with pytest.raises(ValueError):
        rn.step(None, None, None, 0)


def test_clipping_at_both_ends():
    rn = RunningNorm(2, 4, 0.99, clip_obs=1.5, clip_rew=0.25)
    x = np.array([[-100.0, 100.0], [0.0, 0.0], [1.0, -1.0], [0.5, 0.25]], dtype=np.float32)
    o, r = rn.step(x, np.array([-50.0, 50.0, 0.0, 0.01], np.float32), np.zeros(4), 0)
    assert o.dtype == r.dtype == np.float32
    assert o[0].tolist() == [-1.5, 1.5] and abs(o[1:]).max() < 1.5
    assert r[:2].tolist() == [-0.25, 0.25] and r[2] == 0.0 and 0 < r[3] < 0.25


def test_a_constant_feature_stays_zero():
    """Pendulum's fourth float is always 0: mean 0, var -> 1e-4 / count, the output exactly 0; a constant 1 (Point's eighth)
    goes to (1 - mean) / sqrt(var + eps), finite and inside the clip"""
    rn = RunningNorm(4, 300, 0.99)
    g = np.random.default_rng(2)
    for k in range(20):
        x = g.standard_normal((300, 4)).astype(np.float32)
        x[:, 3] = 0.0
        x[:, 2] = 1.0
        o, _ = rn.step(x, None, None, 0)
        assert (o[:, 3] == 0.0).all() and np.isfinite(o).all() and abs(o[:, 2]).max() <= 10.0
    assert rn.obs_mean[3] == 0.0 and 0.0 < rn.obs_var[3] < 1e-7


def test_state_dict_round_trip():
    g = np.random.default_rng(3)
    a = RunningNorm(5, 9, 0.97, eps=1e-6, clip_obs=4, clip_rew=3)
    for k in range(4):
        a.step(g.standard_normal((9, 5)).astype(np.float32), g.standard_normal(9).astype(np.float32), g.uniform(size=9) < 0.3, 0)
    sd = a.state_dict()
    b = RunningNorm(5, 9, 0.5).load_state_dict(sd)
    assert b.to_block().tobytes() == a.to_block().tobytes()
    assert (b.gamma, b.eps, b.clip_obs, b.clip_rew) == (0.97, 1e-6, 4.0, 3.0)
    c = RunningNorm(5, 9, 0.5).from_block(a.to_block())
    assert c.to_block().tobytes() == a.to_block().tobytes() and a.to_block().shape == (4 + 10 + 9,)
    x, r, d = g.standard_normal((9, 5)).astype(np.float32), g.standard_normal(9).astype(np.float32), np.zeros(9)
    (oa, ra), (ob, rb) = a.step(x, r, d, 0), b.step(x, r, d, 0)
    assert oa.tobytes() == ob.tobytes() and ra.tobytes() == rb.tobytes()
    sd["ret"][0] = 123.0                       # the dict holds copies
    assert a.ret[0] != 123.0
    with pytest.raises(ValueError):
        RunningNorm(5, 8, 0.5).load_state_dict(sd)
    with pytest.raises(ValueError):
        RunningNorm(4, 9, 0.5).from_block(a.to_block())


def test_frozen_mode_writes_nothing():
    g = np.random.default_rng(4)
    rn = RunningNorm(3, 5, 0.99)
    rn.step(g.standard_normal((5, 3)).astype(np.float32), g.standard_normal(5).astype(np.float32), np.zeros(5), 0)
    before = rn.to_block().tobytes()
    x = g.standard_normal((2, 3)).astype(np.float32)
    o, r = rn.step(x, None, None, 1, update=False)
    assert rn.to_block().tobytes() == before and r is None
    want = np.clip((x.astype(np.float64) - rn.obs_mean) / np.sqrt(rn.obs_var + rn.eps), -10, 10).astype(np.float32)
    assert o.tobytes() == want.tobytes() and rn.normalize_obs(x).tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        rn.step(x, np.zeros(2, np.float32), np.zeros(2), 1, update=False)


def test_bad_settings_are_refused():
    for kw in (dict(L=0), dict(L=65), dict(B_pool=0), dict(eps=0.0), dict(clip_obs=0), dict(clip_rew=-1)):
        with pytest.raises(ValueError):
            RunningNorm(**dict(dict(L=4, B_pool=2, gamma=0.99), **kw))


# ---------------------------------------------------------------- what train() and the Runner refuse before any GPU work
def _hyps(tmp_path, **kw):
    return dict(dict(exp_name="vecnorm", main_path=str(tmp_path), model="FCModel", env_type="Pendulum-device", n_envs=2,
                     n_rollouts=2, n_tsteps=2, n_frame_stack=2, max_tsteps=1e9, seed=1, h_size=16, norm_obs=True,
                     norm_rewards=True), **kw)


@pytest.mark.parametrize("kw,key", [(dict(env_type="Pendulum-host", env_pool="serial"), "norm_obs"),
                                    (dict(env_type="Pendulum-host", env_pool="serial", norm_obs=False), "norm_rewards"),
                                    (dict(env_type="Pong-device", model="A3CModel"), "norm_obs"),
                                    (dict(env_type="Breakout-device", model="ConvModel", norm_rewards=False), "norm_obs"),
                                    (dict(env_type="Snake-device", model="A3CModel", norm_obs=False), "norm_rewards"),
                                    (dict(env_type="Pong-v0", norm_obs=False), "norm_rewards"),
                                    (dict(norm_clip_obs=0.0), "norm_clip_obs"), (dict(norm_clip_rew=-1), "norm_clip_rew"),
                                    (dict(norm_eps=0), "norm_eps")])
def test_train_refuses_what_the_normaliser_does_not_cover(kw, key, tmp_path):
    from a2c_amd.training import train
    with pytest.raises(ValueError, match=key):
        train(None, _hyps(tmp_path, **kw), verbose=False, max_epochs=1)
    assert not list(tmp_path.iterdir()), "nothing was written"


def test_norm_settings_of_hyps():
    from a2c_amd.vecnorm import norm_settings
    assert norm_settings(dict(gamma=0.9)) is None and norm_settings(dict(norm_obs=False, norm_rewards=0)) is None
    s = norm_settings(dict(norm_obs=True, gamma=0.9))
    assert s == dict(obs=True, rewards=False, clip_obs=10.0, clip_rew=10.0, eps=1e-8)
    s = norm_settings(dict(norm_rewards=True, norm_clip_obs=5, norm_clip_rew=2, norm_eps=1e-4))
    assert s == dict(obs=False, rewards=True, clip_obs=5.0, clip_rew=2.0, eps=1e-4)


def test_runner_refuses_a_host_pool_and_pixel_frames():
    """the checks come before the first device allocation"""
    from a2c_amd.vecnorm import check_runner

    class Net:
        is_recurrent = False

    class Pool:
        frame_shape = (1, 4)

        def device_step_post(self):
            pass
    check_runner(dict(norm_obs=True), Pool(), Net(), stepper=False)
    with pytest.raises(ValueError, match="norm_obs"):
        check_runner(dict(norm_obs=True), object(), Net(), stepper=False)             # a host env pool
    P2 = type("P2", (Pool,), dict(frame_shape=(1, 80, 72)))
    with pytest.raises(ValueError, match="norm_rewards"):
        check_runner(dict(norm_rewards=True), P2(), Net(), stepper=False)             # pixel frames
    P3 = type("P3", (Pool,), dict(frame_shape=(1, 65)))
    with pytest.raises(ValueError, match="norm_obs"):
        check_runner(dict(norm_obs=True, norm_rewards=True), P3(), Net(), stepper=False)      # L > 64
    with pytest.raises(ValueError, match="norm_obs"):
        check_runner(dict(norm_obs=True), Pool(), Net(), stepper=True)                # a net on the one-launch step kernel
    check_runner(dict(), object(), Net(), stepper=True)                               # keys absent: nothing to refuse
    check_runner(dict(), object(), Net(), stepper=True, ranks=4)


class _Net:
    is_recurrent = False


class _VectorPool:
    frame_shape = (1, 4)

    def device_step_post(self):
        pass


def test_runner_refuses_a_sharded_run_above_one_rank(monkeypatch):
    """``ranks`` as the caller's Shard.world; None: the initialised process group's size.  WORLD_SIZE alone is not read"""
    import torch.distributed as dist
    from a2c_amd.vecnorm import check_runner
    with pytest.raises(ValueError, match="norm_obs"):
        check_runner(dict(norm_obs=True), _VectorPool(), _Net(), False, ranks=2)
    with pytest.raises(ValueError, match="norm_rewards"):
        check_runner(dict(norm_rewards=True), _VectorPool(), _Net(), False, ranks=8)
    check_runner(dict(norm_obs=True, norm_rewards=True), _VectorPool(), _Net(), False, ranks=1)
    # no ranks given, no process group: one rank, whatever a launcher left in the environment
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert not dist.is_initialized()
    check_runner(dict(norm_rewards=True), _VectorPool(), _Net(), False)
    # ... and an initialised group above one rank is taken for a sharded run
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(ValueError, match="norm_rewards"):
        check_runner(dict(norm_rewards=True), _VectorPool(), _Net(), False)
    with pytest.raises(ValueError, match="norm_obs"):
        check_runner(dict(norm_obs=True), _VectorPool(), _Net(), False)
    check_runner(dict(norm_obs=True), _VectorPool(), _Net(), False, ranks=1)          # the caller knows better
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 1)
    check_runner(dict(norm_obs=True), _VectorPool(), _Net(), False)


def test_runner_hands_its_ranks_to_the_check():
    """Runner(ranks=...) reaches check_runner: start() refuses before the first device allocation of the normaliser"""
    from a2c_amd.runner import Runner

    class Net(_Net):
        _dev = "cpu"
        output_space = 1
        is_discrete = False

        def _ensure_device(self):
            pass
    hyps = dict(norm_obs=True, n_frame_stack=2, gamma=0.99, action_shift=0, env_type="Pendulum-device")
    class Pool(_VectorPool):
        def __len__(self):
            return 3

        def device_step(self):
            pass
    r = Runner({}, hyps, None, None, None, env_pool=Pool(), ranks=2)
    with pytest.raises(ValueError, match="norm_obs.*sharded"):
        r.start(Net())
    assert r.vecnorm is None
