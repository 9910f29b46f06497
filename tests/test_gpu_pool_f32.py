"""Continuous actions over the process env pool on the MI355X: a2c_gauss_head_publish against a2c_gauss_head (bit-identical
actions, the float action granules and doorbells it stores, guard words around them, the step-counter wrap), rollouts of
FCModel / GRUFCModel over ProcessEnvPool(action_dim=n) against tests/golden/g10_continuous.npz and against the serial
HostEnvPool (device relay and memcpy ingest, per-step graphs on and off, later rollouts on the same Runner), the refusals,
the torch-ops path and a short train() with env_pool="process_f32"."""
import functools
import os

import numpy as np
import pytest
import torch

import a2c_amd
from a2c_amd import ops
from a2c_amd._lib import A2CKernelError
from a2c_amd.hostpool import ProcessEnvPool, ThreadEnvPool, pool_lib
from a2c_amd.runner import HostEnvPool, Runner
import cont_cases as CC

pytestmark = pytest.mark.gpu
GUARD = 0x5a5a5a5a5a5a5a5a


def _net(kind, n, h):
    net = getattr(a2c_amd, kind)(list(CC.STATE_SHAPE), n, h_size=h, is_discrete=False)
    net.load_state_dict(CC.state_dict(kind, n, h, CC.RAW_BIAS[n]))
    return net.cuda()


def _close(name, got, want, atol=1e-5, rtol=1e-5):      # the comparison of tests/test_gpu_continuous.py
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    np.testing.assert_allclose(got, np.asarray(want, np.float64), atol=atol, rtol=rtol, err_msg=name)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------------------------------------------------ 6. kernel
def _kernel_inputs(B, n):
    g = torch.Generator().manual_seed(1000 * B + n)
    heads = torch.randn(B, 2 * n + 1, generator=g) * 1.5
    raw = heads[:, n:2 * n]
    # columns in the manner of cont_cases.RAW_BIAS: softplus's identity branch (> 20, and 20 itself), the tiny-sigma branch
    picks = torch.tensor([24.0, 21.5, 20.0, 20.5, -9.0, -12.0, -3.4, 0.2])
    for j in range(n):
        if j % 3 != 2:
            raw[:, j] = picks[(j + B) % len(picks)] + 0.01 * raw[:, j]
    eps = torch.randn(B, n + 1, generator=g)
    return heads.cuda(), eps.cuda()[:, :n]


def _run_head(B, n, heads, eps, publish, seq_base=None, seq_off=0, null_cmd=False):
    sigma = torch.full((B, n), -7.0, device="cuda")
    acts = torch.full((B, n + 3), -7.0, device="cuda")
    stride = n + 2
    act = torch.full((B * stride + 5,), GUARD, dtype=torch.int64, device="cuda")
    cmd = torch.full((B + 5,), GUARD, dtype=torch.int64, device="cuda")
    if publish:
        ops.gauss_head_publish(heads, n, B, eps, acts.data_ptr(), n + 3, act.data_ptr(), stride,
                               0 if null_cmd else cmd.data_ptr(), seq_base, seq_off, sigma=sigma)
    else:
        ops.gauss_head(heads, n, B, sigma=sigma, eps=eps, actions_ptr=acts.data_ptr(), act_ld=n + 3)
    torch.cuda.synchronize()
    return sigma, acts, act, cmd


@pytest.mark.parametrize("n", [1, 2, 6, 33, 64])
@pytest.mark.parametrize("B", [1, 3, 65, 257])
def test_gauss_head_publish_kernel(B, n):
    heads, eps = _kernel_inputs(B, n)
    assert heads.stride(0) == 2 * n + 1 and eps.stride(0) == n + 1
    s0, a0, act0, cmd0 = _run_head(B, n, heads, eps, publish=False)
    assert (act0 == GUARD).all() and (cmd0 == GUARD).all()
    assert float(s0.min()) > 0 and (a0[:, n:] == -7.0).all()
    stride = n + 2
    base = 0xfffffffe
    seq_base = torch.tensor([base - (1 << 32)], dtype=torch.int32, device="cuda")
    for seq_off in (0, 1, 2, 5):                         # the step number wraps modulo 2^32
        seq = (base + seq_off) & 0xffffffff
        s1, a1, act, cmd = _run_head(B, n, heads, eps, publish=True, seq_base=seq_base, seq_off=seq_off)
        assert torch.equal(s1, s0) and torch.equal(a1, a0)               # bit-identical to a2c_gauss_head
        bits = a1[:, :n].contiguous().cpu().numpy().view(np.uint32).astype(np.uint64)
        g = _u64(act)
        rows = g[:B * stride].reshape(B, stride)
        assert np.array_equal(rows[:, :n], (np.uint64(seq) << np.uint64(32)) | bits), seq_off
        assert (rows[:, n:] == GUARD).all() and (g[B * stride:] == GUARD).all()       # nothing outside the granules
        c = _u64(cmd)
        assert (c[:B] == ((seq << 32) | n)).all() and (c[B:] == GUARD).all()
    # cmd == NULL: a2c_gauss_head, neither buffer is touched
    s2, a2, act, cmd = _run_head(B, n, heads, eps, publish=True, seq_base=seq_base, seq_off=1, null_cmd=True)
    assert torch.equal(s2, s0) and torch.equal(a2, a0)
    assert (act == GUARD).all() and (cmd == GUARD).all()


def test_gauss_head_publish_refuses_bad_arguments():
    B, n = 4, 2
    heads, eps = _kernel_inputs(B, n)
    seq_base = torch.zeros(1, dtype=torch.int32, device="cuda")
    acts = torch.zeros(B, n, device="cuda")
    act = torch.full((B * n,), GUARD, dtype=torch.int64, device="cuda")
    cmd = torch.full((B,), GUARD, dtype=torch.int64, device="cuda")
    wide = torch.zeros(B, 131, device="cuda")
    for bad_n, h in ((65, wide), (0, heads)):            # n outside 1 .. A2C_GAUSS_MAX_N: A2C_ERR_ARG, nothing launched
        with pytest.raises(A2CKernelError, match="invalid argument"):
            ops.gauss_head_publish(h, bad_n, B, eps, acts.data_ptr(), n, act.data_ptr(), n, cmd.data_ptr(), seq_base, 0)
    with pytest.raises(A2CKernelError):                  # act_stride < n
        ops.gauss_head_publish(heads, n, B, eps, acts.data_ptr(), n, act.data_ptr(), n - 1, cmd.data_ptr(), seq_base, 0)
    with pytest.raises(A2CKernelError):                  # a doorbell without granules
        ops.gauss_head_publish(heads, n, B, eps, acts.data_ptr(), n, 0, n, cmd.data_ptr(), seq_base, 0)
    with pytest.raises(A2CKernelError):                  # ... without the step counter
        ops.gauss_head_publish(heads, n, B, eps, acts.data_ptr(), n, act.data_ptr(), n, cmd.data_ptr(), None, 0)
    torch.cuda.synchronize()
    assert (act == GUARD).all() and (cmd == GUARD).all() and not acts.any()


# ------------------------------------------------------------------------------------------------- 7. / 8. rollouts
def _datas(N, n, recurrent, h):
    D = dict(states=torch.zeros(N, *CC.STATE_SHAPE, device="cuda"), deltas=torch.zeros(N, device="cuda"),
             rewards=torch.zeros(N, device="cuda"), dones=torch.zeros(N, device="cuda"),
             actions=torch.zeros(N, n, device="cuda"))
    if recurrent:
        D["h_states"] = torch.zeros(N, h, device="cuda")
    return D


def _env_kwargs(n, B):
    return [dict(n=n, env_id=j, done_period=4 + j, prepped=True) for j in range(B)]


def _process_pool(n, B):
    return ProcessEnvPool(CC.ContEnv, B, env_kwargs=_env_kwargs(n, B), n_workers=2, action_dim=n)


_SERIAL = {}


def _serial_rollouts(golden, case, rounds):
    """the same envs and noise on the serial HostEnvPool: the rollout buffers after each of `rounds` rollouts (computed
    once per case, never modified)"""
    if case[0] not in _SERIAL:
        name, kind, n, h, T, B = case
        net = _net(kind, n, h)
        D = _datas(T * B, n, net.is_recurrent, h)
        eps = torch.from_numpy(golden["g10_continuous"][f"{name}_noise"]).cuda()
        hyps = CC.cont_hyps(n_tsteps=T, n_rollouts=B)
        r = Runner(D, hyps, None, None, None, env_pool=HostEnvPool([CC.ContEnv(**kw) for kw in _env_kwargs(n, B)]),
                   normal_fn=lambda t, Bn, e0: eps[t, e0:e0 + Bn])
        out = []
        for _ in range(max(rounds, ROUNDS)):
            r.rollout(net, list(range(B)), hyps)
            torch.cuda.synchronize()
            out.append({k: v.clone() for k, v in D.items()})
        _SERIAL[case[0]] = out
    return _SERIAL[case[0]]


ROUNDS = 3      # graphs on: the first rollout runs eagerly, the second is captured, the third is a pure replay


def _pool_rollouts(golden, case, ingest, graphs, rounds=ROUNDS, check=True):
    name, kind, n, h, T, B = case
    g = golden["g10_continuous"]
    net = _net(kind, n, h)
    D = _datas(T * B, n, net.is_recurrent, h)
    eps = torch.from_numpy(g[f"{name}_noise"]).cuda()
    hyps = CC.cont_hyps(n_tsteps=T, n_rollouts=B, rollout_graphs=graphs, env_timeout_s=20.0)
    pool = _process_pool(n, B)
    r = Runner(D, hyps, None, None, None, env_pool=pool, ingest=ingest, normal_fn=lambda t, Bn, e0: eps[t, e0:e0 + Bn])
    keys = ("states", "actions", "rewards", "dones", "deltas") + (("h_states",) if net.is_recurrent else ())
    serial = _serial_rollouts(golden, case, rounds) if check else None
    out = []
    try:
        for rnd in range(rounds):
            r.rollout(net, list(range(B)), hyps)
            r.finish()
            assert int(pool.seq) == (rnd + 1) * T
            out.append({k: v.clone() for k, v in D.items()})
            if not check:
                continue
            if rnd == 0:      # the recorded reference rollout, compared as test_rollout_matches_reference does
                for k in keys:
                    _close(f"{name} {k}", D[k], g[f"{name}_{k}"], atol=1e-5, rtol=1e-5)
            for k in ("states", "actions", "rewards", "dones"):      # ... and the serial pool, exactly
                assert torch.equal(D[k], serial[rnd][k]), (name, ingest, graphs, rnd, k)
            for k in keys[4:]:
                _close(f"{name} round {rnd} {k}", D[k], serial[rnd][k].cpu().numpy(), atol=1e-5, rtol=1e-5)
        assert r.cont and pool.header.act_dim == n
        assert int(pool.header.episodes) > 0
    finally:
        r.close()
    return out


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("ingest", ["relay", "memcpy"])
@pytest.mark.parametrize("case", CC.ROLLOUT_CASES, ids=[c[0] for c in CC.ROLLOUT_CASES])
def test_rollouts_over_the_process_pool(golden, case, ingest, graphs):
    """the first rollout against the recorded reference and the serial pool, then two more on the same Runner (the step
    counter goes on; with graphs on these are the capture and a replay of the per-step segments) against the serial pool's"""
    _pool_rollouts(golden, case, ingest, graphs)


def test_rollout_without_step_graphs(golden, monkeypatch):
    """A2C_NO_STEP_GRAPHS=1: the stepwise path (memcpy ingest: D2H of the float rows, a2c_pool_post_actions_f32)"""
    monkeypatch.setenv("A2C_NO_STEP_GRAPHS", "1")
    _pool_rollouts(golden, CC.ROLLOUT_CASES[0], None, False, rounds=2)


# ---------------------------------------------------------------------------------------------------------- 9. refusals
def test_runner_refusals():
    from a2c_amd.synthetic import TapeEnv
    n, B, T = 2, 2, 3
    net = _net("FCModel", n, 16)
    hyps = CC.cont_hyps(n_tsteps=T, n_rollouts=B)
    D = _datas(T * B, n, False, 16)
    for kw in (dict(), dict(action_dim=n + 1)):          # an int pool; a pool of another dimension
        pool = ProcessEnvPool(CC.ContEnv, B, env_kwargs=_env_kwargs(n, B), n_workers=2, **kw)
        r = Runner(D, hyps, None, None, None, env_pool=pool)
        with pytest.raises(ValueError, match="continuous"):
            r.start(net)
        assert pool.region is None                       # refused before any worker was started
    envs = [TapeEnv(env_id=j, length=5) for j in range(B)]
    tpool = ThreadEnvPool.from_tape_envs(envs, n_threads=1)
    try:
        with pytest.raises(ValueError, match="continuous"):
            Runner(D, hyps, None, None, None, env_pool=tpool).start(net)
        assert tpool.region is None
    finally:
        for p in tpool.env_ptrs:
            pool_lib().a2c_tape_env_destroy(p)
        tpool.env_ptrs = []
    # and a discrete net has no use for float action granules
    dnet = a2c_amd.FCModel(list(CC.STATE_SHAPE), 3, h_size=16).cuda()
    Dd = dict(D, actions=torch.zeros(T * B, dtype=torch.int64, device="cuda"))
    pool = _process_pool(n, B)
    with pytest.raises(ValueError, match="action_dim"):
        Runner(Dd, CC.cont_hyps(n_tsteps=T, n_rollouts=B, is_discrete=True), None, None, None, env_pool=pool).start(dnet)
    assert pool.region is None


# ------------------------------------------------------------------------------------------------------ 10. torch ops
def test_torch_ops_path_is_bit_identical(golden, monkeypatch):
    if not os.path.exists(os.path.join(os.path.dirname(ops.__file__), "liba2c_torch_ops.so")):
        pytest.fail("liba2c_torch_ops.so was not built")
    case = CC.ROLLOUT_CASES[0]
    ref = _pool_rollouts(golden, case, "relay", False, rounds=2)
    B, n = 65, 6
    heads, eps = _kernel_inputs(B, n)
    seq_base = torch.tensor([41], dtype=torch.int32, device="cuda")
    k0 = _run_head(B, n, heads, eps, publish=True, seq_base=seq_base, seq_off=3)
    monkeypatch.setenv("A2C_TORCH_OPS", "1")
    assert hasattr(ops.load_torch_ops(), "abi_gauss_head_publish")
    cnt = lambda: ops.torch_abi().stats["by_name"].get("a2c_gauss_head_publish", 0)
    before = cnt()
    k1 = _run_head(B, n, heads, eps, publish=True, seq_base=seq_base, seq_off=3)
    assert cnt() == before + 1                           # device tensors: the launch went through the dispatcher
    for a, b in zip(k0, k1):
        assert torch.equal(a, b)
    # the rollout: the launches with addresses inside the pinned region fall back to ctypes call by call, the rest go
    # through torch.ops.a2c_mi355x.abi_*; same C functions, same arguments
    launches = ops.torch_abi().stats["torch_ops"]
    got = _pool_rollouts(golden, case, "relay", False, rounds=2)
    assert ops.torch_abi().stats["torch_ops"] > launches
    for rnd in range(2):
        for k in ref[rnd]:
            assert torch.equal(ref[rnd][k], got[rnd][k]), (rnd, k)


# ---------------------------------------------------------------------------------------------------------- 11. train()
# env_fn(j) -> ContEnv(2, j, prepped=True); picklable without cloudpickle, and the workers need not import this module
_cont_env = functools.partial(CC.ContEnv, 2, prepped=True)


def test_train_process_f32(tmp_path):
    from a2c_amd.training import train
    n = 2
    hyps = dict(exp_name="c", main_path=str(tmp_path), model="FCModel", env_type="ContEnv", n_envs=2, n_rollouts=2,
                n_tsteps=3, max_tsteps=1e9, action_size=n, is_discrete=False, n_frame_stack=CC.C_STACK, h_size=32,
                seed=3, env_pool="process_f32", n_env_workers=2)
    infos = []
    best = train(None, hyps, verbose=False, env_fn=_cont_env, max_epochs=2,
                 on_epoch=lambda e, upd, D: infos.append((dict(upd.info), D["actions"].shape, D["actions"].dtype)))
    assert len(infos) == 2 and np.isfinite(best)
    for info, shape, dtype in infos:
        assert all(np.isfinite(v) for v in info.values()), info
        assert tuple(shape) == (6, n) and dtype == torch.float32
    sd = torch.load(os.path.join(str(tmp_path), "c", "c_0", "net.p"))
    assert tuple(sd["action_out.weight"].shape) == (2 * n, 32)
    assert os.path.exists(os.path.join(str(tmp_path), "c", "c_0", "optim.p"))
    # a discrete env has no float actions to carry ...
    from cases import F32FakeEnv
    dh = dict(hyps, exp_name="d", action_size=3, is_discrete=True, n_frame_stack=2)
    with pytest.raises(ValueError, match="process_f32"):
        train(None, dh, verbose=False, env_fn=lambda j: F32FakeEnv(env_id=j), max_epochs=1)
    # ... and "process" keeps meaning the int32 command-word pool
    with pytest.raises(ValueError, match="serial"):
        train(None, dict(hyps, exp_name="e", env_pool="process"), verbose=False, env_fn=_cont_env, max_epochs=1)
