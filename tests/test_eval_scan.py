"""a2c_eval_scan (the first-episode scan of DeviceStatsRunner): its argument checks and ``train()``'s ``eval_pool`` key without
a GPU; -m gpu: the kernel against a NumPy loop written here, step by step in np.float32 -- every comparison is exact."""
import itertools

import numpy as np
import pytest
import torch

DEV = "cuda"


# ---------------------------------------------------------------- no GPU
def test_argument_checks_return_err_arg_without_launching():
    """every refusal comes back before anything touches the device: the pointers are not even memory"""
    from a2c_amd import _lib
    lib = _lib.load()
    P = 4096        # any non-NULL address: a refused call reads none of them
    good = dict(rewards=P, dones=P, T=8, K=8, E=3, t0=0, max_steps=10, ep_rew=P, ep_len=P, active=P, n_active=P)
    order = list(good)
    bad = [{k: None} for k in ("rewards", "dones", "ep_rew", "ep_len", "active", "n_active")]
    bad += [dict(E=0), dict(E=-4), dict(K=0), dict(K=-1), dict(T=7), dict(T=0), dict(t0=-1), dict(max_steps=0), dict(max_steps=-5)]
    for o in bad:
        a = dict(good, **o)
        assert lib.a2c_eval_scan(*[a[k] for k in order], None) == -1, o
    assert len(_lib.SIGNATURES["a2c_eval_scan"][1]) == len(order) + 1


def _train_hyps(tmp_path, **kw):
    return dict(dict(exp_name="e", main_path=str(tmp_path), model="FCModel", env_type="Pong-device", n_envs=2, n_tsteps=2,
                     seed=1), **kw)


def test_train_refuses_eval_pool_device_off_the_device_worlds(tmp_path, monkeypatch):
    from a2c_amd import pong, training

    def no_pool(*a, **k):
        raise AssertionError("a pool was built")
    monkeypatch.setattr(pong, "DevicePongPool", no_pool)
    monkeypatch.setattr(training, "HostEnvPool", no_pool)
    with pytest.raises(ValueError, match="eval_pool"):
        training.train(None, _train_hyps(tmp_path, env_type="Pong-host", env_pool="serial", eval_pool="device"), verbose=False)
    with pytest.raises(ValueError, match="eval_pool"):
        training.train(None, _train_hyps(tmp_path, eval_pool="device"), verbose=False, eval_env=object())
    with pytest.raises(ValueError, match="eval_pool"):
        training.train(None, _train_hyps(tmp_path, eval_pool="device", action_size=3), verbose=False, env_fn=lambda j: None)
    assert not list(tmp_path.iterdir()), "refused before the save folder was made"


def test_train_refuses_an_unknown_eval_pool(tmp_path):
    from a2c_amd import training
    for v in ("gpu", "Device", 1):
        with pytest.raises(ValueError, match="eval_pool"):
            training.train(None, _train_hyps(tmp_path, eval_pool=v), verbose=False)


# ---------------------------------------------------------------- the kernel
def ref_scan(rewards, dones, T, K, E, t0, max_steps, ep_rew, ep_len, active):
    """the header's definition, one env and one step at a time; fp32 sums in step order -> n_active"""
    for e in range(E):
        for t in range(K):
            if active[e] == 0 or t0 + t >= max_steps:
                break
            ep_rew[e] = np.float32(ep_rew[e] + rewards[e * T + t])
            ep_len[e] += 1
            if dones[e * T + t] != 0:
                active[e] = 0
    return int((active[:E] != 0).sum())


def make_inputs(E, K, T, fp_rewards, seed):
    """rows of T with K steps played (the T - K tail holds values that must not be read: huge rewards, dones set); dones
    with p = 0.2 and nonzero values other than 1; every fourth env never done; every fifth enters closed, with a score"""
    rs = np.random.RandomState(seed)
    if fp_rewards:
        rew = rs.choice(np.array([0.1, 1e-3, 3.7, -0.3, 0.0, 1e4], dtype=np.float32), size=(E, T))
    else:
        rew = rs.randint(-2, 4, size=(E, T)).astype(np.float32)
    don = (rs.rand(E, T) < 0.2).astype(np.float32) * rs.choice(np.array([1.0, 2.0, -1.0, 0.5], dtype=np.float32), size=(E, T))
    don[::4] = 0.0
    rew[:, K:], don[:, K:] = 1e30, 1.0
    active = np.ones(E, dtype=np.int32)
    active[2::5] = 0
    active[1::7] = 3                                       # active is "nonzero"
    ep_rew = np.where(active == 0, np.float32(7.25), rs.choice(np.array([0.0, 0.7], dtype=np.float32), size=E)).astype(np.float32)
    ep_len = np.where(active == 0, 11, rs.randint(0, 3, size=E)).astype(np.int32)
    return rew.reshape(-1), don.reshape(-1), ep_rew, ep_len, active


def run_both(rew, don, T, K, E, t0, max_steps, ep_rew, ep_len, active, garbage=-12345):
    from a2c_amd import ops
    d = [torch.from_numpy(np.array(x)).to(DEV) for x in (rew, don, ep_rew, ep_len, active)]
    n_active = torch.full((1,), garbage, dtype=torch.int32, device=DEV)
    ops.eval_scan(d[0], d[1], T, K, E, t0, max_steps, d[2], d[3], d[4], n_active)
    w = [np.array(x) for x in (ep_rew, ep_len, active)]
    n = ref_scan(rew, don, T, K, E, t0, max_steps, *w)
    return d, n_active, w, n


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 257, 1000])
def test_scan_equals_the_numpy_loop(E, K, pad):
    T, t0 = K + pad, 5
    # max_steps: t0 + K below it, equal to it, straddling it (K = 1 has no straddle: that cap closes the chunk), beyond it
    caps = dict(below=t0 + K + 3, equal=t0 + K, straddle=t0 + K // 2, beyond=t0 - 2)
    for (cname, cap), fp in itertools.product(caps.items(), (False, True)):
        rew, don, ep_rew, ep_len, active = make_inputs(E, K, T, fp, seed=E * 10 + K)
        d, n_active, w, n = run_both(rew, don, T, K, E, t0, cap, ep_rew, ep_len, active)
        torch.cuda.synchronize()
        what = (E, K, T, cname, fp)
        assert np.array_equal(d[2].cpu().numpy(), w[0]), what
        assert np.array_equal(d[3].cpu().numpy(), w[1]) and np.array_equal(d[4].cpu().numpy(), w[2]), what
        assert int(n_active.item()) == n, what
        assert torch.equal(d[0].cpu(), torch.from_numpy(rew)) and torch.equal(d[1].cpu(), torch.from_numpy(don)), "inputs"
        closed = active == 0
        assert np.array_equal(w[0][closed], ep_rew[closed]) and np.array_equal(w[1][closed], ep_len[closed]), "closed envs"
        if cname in ("beyond",) or (cname == "straddle" and K == 1):
            assert np.array_equal(w[0], ep_rew) and np.array_equal(w[1], ep_len) and n == int((active != 0).sum())
        elif E >= 63:
            assert not np.array_equal(w[1], ep_len) and 0 < n < E, what      # the case shows envs closing and envs playing on
        if fp and cname == "below" and K == 7 and E >= 257:
            # the order of the fp32 sum matters for these rewards: the same steps added in float64 round differently
            wide = ep_rew.astype(np.float64)
            for e, t in itertools.product(range(E), range(K)):
                if active[e] and not (don.reshape(E, T)[e, :t] != 0).any():
                    wide[e] += rew.reshape(E, T)[e, t]
            assert (wide.astype(np.float32) != w[0]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("fp", [False, True])
@pytest.mark.parametrize("E", [7, 257])
def test_two_chained_chunks_equal_one_pass(E, fp):
    from a2c_amd import ops
    K = 7
    T = 2 * K
    for cap in (100, T, K + 3, K, K - 2):       # no cap in reach; at the end; inside chunk 1; between the chunks; inside chunk 0
        rew, don, ep_rew, ep_len, active = make_inputs(E, T, T, fp, seed=E + cap)
        one, n_one, w, n = run_both(rew, don, T, T, E, 0, cap, ep_rew, ep_len, active)
        d = [torch.from_numpy(np.array(x)).to(DEV) for x in (rew, don, ep_rew, ep_len, active)]
        n_active = torch.full((1,), 99, dtype=torch.int32, device=DEV)
        ops.eval_scan(d[0], d[1], T, K, E, 0, cap, d[2], d[3], d[4], n_active)
        first = int(n_active.item())
        ops.eval_scan(d[0][K:], d[1][K:], T, K, E, K, cap, d[2], d[3], d[4], n_active)
        for got, want_dev, want in zip(d[2:], one[2:], w):
            assert torch.equal(got, want_dev) and np.array_equal(got.cpu().numpy(), want), (E, fp, cap)
        assert int(n_active.item()) == int(n_one.item()) == n and first >= n


@pytest.mark.gpu
def test_ops_eval_scan_refuses_short_or_mistyped_buffers():
    from a2c_amd import ops
    E, K = 5, 4
    f = lambda n: torch.zeros(n, device=DEV)
    i = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    ops.eval_scan(f(E * K), f(E * K), K, K, E, 0, 10, f(E), i(E), i(E), i(1))
    with pytest.raises(ValueError):
        ops.eval_scan(f(E * K - 1), f(E * K), K, K, E, 0, 10, f(E), i(E), i(E), i(1))
    with pytest.raises(ValueError):
        ops.eval_scan(f(E * K), f(E * K), K, K, E, 0, 10, f(E), i(E - 1), i(E), i(1))
    with pytest.raises(TypeError):
        ops.eval_scan(f(E * K), f(E * K), K, K, E, 0, 10, f(E), i(E), f(E), i(1))
    with pytest.raises(RuntimeError):
        ops.eval_scan(torch.zeros(E * K), f(E * K), K, K, E, 0, 10, f(E), i(E), i(E), i(1))
