"""Continuous (Gaussian) actions on the MI355X: the a2c_gauss_* kernels against a float64 autograd statement of the loss,
FCModel / GRUFCModel forwards, rollouts and updates against tests/golden/g10_continuous.npz (recorded from the reference),
graphed replay, the torch-ops path and a short train()."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import a2c_amd
from a2c_amd import ops
from a2c_amd._lib import A2CKernelError
from a2c_amd.runner import HostEnvPool, Runner
from a2c_amd.updater import Updater
import cont_cases as CC

pytestmark = pytest.mark.gpu
R2PI = float(np.sqrt(2 * np.pi))


def _net(kind, n, h, raw_bias=None):
    net = getattr(a2c_amd, kind)(list(CC.STATE_SHAPE), n, h_size=h, is_discrete=False)
    net.load_state_dict(CC.state_dict(kind, n, h, raw_bias if raw_bias is not None else CC.RAW_BIAS[n]))
    return net.cuda()


def _close(name, got, want, atol=1e-5, rtol=1e-5):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    np.testing.assert_allclose(got, np.asarray(want, np.float64), atol=atol, rtol=rtol, err_msg=name)


# ---------------------------------------------------------------------------------------------------------- kernels
def _rand_heads(N, n, seed):
    g = torch.Generator().manual_seed(seed)
    heads = torch.randn(N, 2 * n + 1, generator=g) * 1.5
    raw = heads[:, n:2 * n]
    # every regime: softplus identity (> 20, and exactly 20), tiny sigma (both clamps), around the sigma^2 clamp
    picks = torch.tensor([25.0, 20.0, 20.5, -9.0, -12.0, -3.43, -3.4, 0.0])
    m = torch.rand(N, n, generator=g) < 0.3
    raw[m] = picks[torch.randint(0, len(picks), (int(m.sum()),), generator=g)]
    return heads


def _reference_loss(heads, vals, acts, advs, rets, n, norm, pi_coef, val_coef, entr_coef):
    """float64 autograd statement of the Gaussian loss the issue specifies (F.mse_loss over the whole (N, n) block, the
    n == 1 outer-product broadcast of the advantages)"""
    h = heads.double().clone().requires_grad_(True)
    mu, raw, v = h[:, :n], h[:, n:2 * n], h[:, 2 * n]
    sigma = F.softplus(raw) + 1e-4
    a = advs.double()
    if norm:
        a = (a - a.mean()) / (a.std() + 1e-6)
    mse = ((mu - acts.double()) ** 2).mean()
    ell = torch.log(torch.clamp(R2PI * sigma, min=1e-3))
    log_ps = -mse / (2 * torch.clamp(sigma ** 2, min=1e-3)) - ell
    if n == 1:
        pi_loss = pi_coef * -(log_ps * a).mean()               # (N,1) * (N,) -> (N, N)
    else:
        pi_loss = pi_coef * -(log_ps * a[:, None]).mean()
    val_loss = val_coef * ((v - rets.double()) ** 2).mean()
    entr = -entr_coef * ell.mean()
    (pi_loss + val_loss - entr).backward()
    return float(pi_loss.detach()), float(val_loss.detach()), float(entr.detach()), h.grad


@pytest.mark.parametrize("n", [1, 2, 6, 32])
def test_gauss_head_matches_torch(n):
    B = 300
    heads = _rand_heads(B, n, 1 + n).cuda()
    eps = torch.randn(B, n, generator=torch.Generator().manual_seed(7)).cuda()
    sigma = torch.empty(B, n, device="cuda")
    acts = torch.zeros(B, 3 * n, device="cuda")              # strided rows, like datas['actions'] rows T apart
    ops.gauss_head(heads, n, B, sigma=sigma, eps=eps, actions_ptr=acts.data_ptr(), act_ld=3 * n)
    torch.cuda.synchronize()
    want_s = F.softplus(heads[:, n:2 * n]) + 1e-4
    _close("sigma", sigma, want_s.cpu(), atol=0, rtol=2e-7)
    want_a = heads[:, :n] + sigma * eps                      # two torch ops on the kernel's sigma: bit-identical
    assert torch.equal(acts[:, :n], want_a)
    assert torch.count_nonzero(acts[:, n:]) == 0
    with pytest.raises(A2CKernelError):         # n above A2C_GAUSS_MAX_N: A2C_ERR_ARG, nothing launched
        ops.gauss_head(heads, 65, B, sigma=sigma)


@pytest.mark.parametrize("N,n,norm", [(300, 1, False), (300, 1, True), (1000, 3, True), (1000, 3, False), (77, 6, True),
                                      (5000, 2, True)])
def test_gauss_loss_kernels_match_autograd(N, n, norm):
    heads = _rand_heads(N, n, 100 + N + n)
    g = torch.Generator().manual_seed(N * 7 + n)
    acts = torch.randn(N, n, generator=g) * 1.3
    advs, rets = torch.randn(N, generator=g), torch.randn(N, generator=g)
    pi_c, val_c, ent_c = 1.0, 0.5, 0.01
    pi, vl, en, grad = _reference_loss(heads, heads[:, 2 * n], acts, advs, rets, n, norm, pi_c, val_c, ent_c)
    hd, ad, av, rt = heads.cuda(), acts.cuda(), advs.cuda(), rets.cuda()
    outs = []
    for _ in range(2):
        stats = torch.zeros(8, dtype=torch.float64, device="cuda")
        sums = torch.zeros(6, dtype=torch.float64, device="cuda")
        adv_sums = None
        if norm:
            adv_sums = stats[0:2]
            ops.moments(av, adv_sums)
        dh = torch.zeros(N, 2 * n + 1, device="cuda")
        ops.gauss_loss_sums(hd[:, :2 * n], hd[:, 2 * n], ad, av, rt, adv_sums, N, n, sums)
        ops.gauss_loss_fwd_bwd(hd[:, :2 * n], hd[:, 2 * n], ad, av, rt, adv_sums, sums, N, n, pi_c, val_c, ent_c,
                               dh[:, :2 * n], dh[:, 2 * n], stats[2:5])
        torch.cuda.synchronize()
        outs.append((stats.clone(), sums.clone(), dh.clone()))
    stats, sums, dh = outs[0]
    for a, b in zip(outs[0], outs[1]):              # deterministic: no atomics on the sums
        assert torch.equal(a, b)
    s = stats.cpu().numpy()
    _close("Pi_Loss", pi_c * -(s[2] / N), pi, atol=1e-5, rtol=1e-5)
    _close("ValLoss", val_c * s[3] / N, vl, atol=1e-5, rtol=1e-5)
    _close("Entropy", -ent_c * s[4] / N, en, atol=1e-6, rtol=1e-5)
    gmax = float(grad.abs().max())
    _close("dheads", dh, grad.numpy(), atol=1e-5 * gmax + 1e-9, rtol=1e-4)


# ----------------------------------------------------------------------------------------------------- model / golden
def test_forwards_match_reference(golden):
    g = golden["g10_continuous"]
    for i, (kind, n, h, B) in enumerate(CC.MODEL_CASES):
        net = _net(kind, n, h)
        x, hin = CC.model_input(i, kind, B, h)
        with torch.no_grad():
            out = net(x.cuda(), hin.cuda()) if hin is not None else net(x.cuda())
        v, (mu, sg) = out[0], out[1]
        _close(f"val{i}", v, g[f"fwd{i}_val"])
        _close(f"mu{i}", mu, g[f"fwd{i}_mu"])
        _close(f"sigma{i}", sg, g[f"fwd{i}_sigma"])
        if hin is not None:
            _close(f"h{i}", out[2], g[f"fwd{i}_h"])


def test_public_forward_is_differentiable():
    net = _net("FCModel", 2, 16, raw_bias=[0.3, -0.7])
    x = CC.model_input(0, "FCModel", 4, 16)[0].cuda()
    for p in net.parameters():
        p.requires_grad_(True)
    v, (mu, sg) = net(x)
    (v.sum() + (mu * 0.5).sum() + (sg ** 2).sum()).backward()
    g = net.action_out.bias.grad.detach().cpu()
    assert torch.isfinite(g).all() and float(g[:2].abs().min()) > 0 and float(g[2:].abs().min()) > 0


@pytest.mark.parametrize("graphs", [True, False])
def test_rollout_matches_reference(golden, monkeypatch, graphs):
    g = golden["g10_continuous"]
    if not graphs:
        monkeypatch.setenv("A2C_NO_STEP_GRAPHS", "1")
    for ci, (name, kind, n, h, T, B) in enumerate(CC.ROLLOUT_CASES):
        net = _net(kind, n, h)
        N = T * B
        D = dict(states=torch.zeros(N, *CC.STATE_SHAPE, device="cuda"), deltas=torch.zeros(N, device="cuda"),
                 rewards=torch.zeros(N, device="cuda"), dones=torch.zeros(N, device="cuda"),
                 actions=torch.zeros(N, n, device="cuda"))
        if net.is_recurrent:
            D["h_states"] = torch.zeros(N, h, device="cuda")
        eps = torch.from_numpy(g[f"{name}_noise"]).cuda()
        envs = [CC.ContEnv(n, env_id=j, done_period=4 + j, prepped=True) for j in range(B)]
        hyps = CC.cont_hyps(n_tsteps=T, n_rollouts=B)
        r = Runner(D, hyps, None, None, None, env_pool=HostEnvPool(envs),
                   normal_fn=lambda t, Bn, e0: eps[t, e0:e0 + Bn])
        r.rollout(net, list(range(B)), hyps)
        torch.cuda.synchronize()
        for k in ("states", "actions", "rewards", "dones", "deltas") + (("h_states",) if net.is_recurrent else ()):
            _close(f"{name} {k}", D[k], g[f"{name}_{k}"], atol=1e-5, rtol=1e-5)
        for j, e in enumerate(envs):          # the env got float (n,) vectors: the recorded action rows
            _close(f"{name} env{j}", np.stack(e.actions), g[f"{name}_actions"][j * T:(j + 1) * T])


def test_host_actions_buffer_and_stats_runner():
    """datas['actions'] on the host (the reference keeps it there) and the lock-step evaluation runner"""
    from a2c_amd.runner import StatsRunner
    n, T, B = 3, 4, 2
    net = _net("FCModel", n, 16, raw_bias=[0.1, -0.5, 1.0])
    N = T * B
    D = dict(states=torch.zeros(N, *CC.STATE_SHAPE, device="cuda"), deltas=torch.zeros(N, device="cuda"),
             rewards=torch.zeros(N, device="cuda"), dones=torch.zeros(N, device="cuda"), actions=torch.zeros(N, n))
    envs = [CC.ContEnv(n, env_id=j, prepped=True) for j in range(B)]
    hyps = CC.cont_hyps(n_tsteps=T, n_rollouts=B)
    r = Runner(D, hyps, None, None, None, env_pool=HostEnvPool(envs))
    r.rollout(net, [0, 1], hyps)
    torch.cuda.synchronize()
    for j, e in enumerate(envs):
        np.testing.assert_array_equal(np.stack(e.actions).astype(np.float32), D["actions"][j * T:(j + 1) * T].numpy())
    sr = StatsRunner(hyps, envs=[CC.ContEnv(n, env_id=j, done_period=3, prepped=True) for j in range(3)])
    assert np.isfinite(sr.rollout(net))


def _update_case(kind, n, h, R_, T, opt, norm, seed, use_bptt=False):
    net = _net(kind, n, h, CC.UPDATE_RAW_BIAS[n])
    hyps = CC.cont_hyps(n_tsteps=T, n_rollouts=R_, optim_type=opt, norm_advs=norm, use_bptt=use_bptt, h_size=h)
    D = {k: v.cuda() for k, v in CC.synth_shared(n, h, R_, T, seed=seed, recurrent=net.is_recurrent).items()}
    return net, Updater(net, hyps), D


@pytest.mark.parametrize("case", CC.UPDATE_CASES, ids=[c[0] for c in CC.UPDATE_CASES])
def test_update_matches_reference(golden, case):
    g = golden["g10_continuous"]
    ci = CC.UPDATE_CASES.index(case)
    name, kind, n, h, R_, T, opt, norm = case
    net, upd, D = _update_case(kind, n, h, R_, T, opt, norm, 1200 + 10 * ci)
    info = upd.update_model(D)
    for k in ("Loss", "Pi_Loss", "ValLoss", "Entropy", "GradNorm"):
        want = float(g[f"{name}_{k}"])
        assert abs(info[k] - want) <= 1e-5 + 1e-5 * abs(want), (k, info[k], want)
    got = torch.cat([p.detach().reshape(-1).cpu() for p in net.parameters()])
    _close(name + " params", got, g[f"{name}_params"], atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("case", CC.BPTT_CASES, ids=[c[0] for c in CC.BPTT_CASES])
def test_bptt_matches_stepped_public_forward(case):
    """Updater.bptt = the public forward stepped over the n_tsteps with h masked by (1 - done); then a BPTT update runs"""
    name, n, h, R_, T, opt, norm = case
    net, upd, D = _update_case("GRUFCModel", n, h, R_, T, opt, norm, 1500, use_bptt=True)
    vals, (mu, sg) = upd.bptt(D["states"], D["h_states"], D["dones"])
    assert vals.shape == (R_ * T,) and mu.shape == (R_ * T, n) and sg.shape == (R_ * T, n)
    S = D["states"].view(R_, T, *CC.STATE_SHAPE)
    hs = D["h_states"].view(R_, T, h)[:, 0]
    keep = 1 - D["dones"].view(R_, T, 1)
    with torch.no_grad():
        for t in range(T):
            v, (m, s), hs = net(S[:, t], hs)
            hs = hs * keep[:, t]
            _close(f"{name} val t{t}", vals.view(R_, T)[:, t], v.view(-1).cpu())
            _close(f"{name} mu t{t}", mu.view(R_, T, n)[:, t], m.cpu())
            _close(f"{name} sigma t{t}", sg.view(R_, T, n)[:, t], s.cpu())
    info = upd.update_model(D)
    assert all(np.isfinite(v) for v in info.values()), info


@pytest.mark.parametrize("kind,use_bptt", [("FCModel", False), ("GRUFCModel", True)])
def test_graphed_update_equals_eager(kind, use_bptt):
    def run(graphed):
        net, upd, D = _update_case(kind, 2, 16, 3, 4, "RMSprop", True, 1600, use_bptt=use_bptt)
        infos = [upd.update_model(D)]
        if graphed:
            rep = upd.capture_update(D)
            infos += [rep(), rep()]
        else:
            infos += [upd.update_model(D), upd.update_model(D)]
        return infos, torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    ie, pe = run(False)
    ig, pg = run(True)
    assert torch.equal(pe, pg)
    assert ie == ig


def test_torch_ops_path_is_bit_identical(monkeypatch):
    def run():
        net, upd, D = _update_case("FCModel", 6, 16, 3, 5, "RMSprop", True, 1700)
        info = upd.update_model(D)
        return info, torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    i0, p0 = run()
    monkeypatch.setenv("A2C_TORCH_OPS", "1")
    if not os.path.exists(os.path.join(os.path.dirname(ops.__file__), "liba2c_torch_ops.so")):
        pytest.fail("liba2c_torch_ops.so was not built")
    before = dict(ops.torch_abi().stats["by_name"])
    i1, p1 = run()
    after = ops.torch_abi().stats["by_name"]
    for k in ("gauss_loss_sums", "gauss_loss_fwd_bwd"):
        cnt = lambda d: sum(v for name, v in d.items() if name.endswith(k))
        assert cnt(after) > cnt(before), (k, after)
    assert torch.equal(p0, p1) and i0 == i1


def test_train_two_epochs_continuous(tmp_path):
    from a2c_amd.training import train
    n = 2
    hyps = dict(exp_name="c", main_path=str(tmp_path), model="FCModel", env_type="ContEnv", n_envs=3, n_rollouts=3,
                n_tsteps=5, max_tsteps=1e9, action_size=n, is_discrete=False, n_frame_stack=CC.C_STACK, h_size=32,
                seed=3)
    infos = []
    best = train(None, hyps, verbose=False, env_fn=lambda j: CC.ContEnv(n, env_id=j, prepped=True), max_epochs=2,
                 on_epoch=lambda e, upd, D: infos.append((dict(upd.info), D["actions"].shape, D["actions"].dtype)))
    assert len(infos) == 2 and np.isfinite(best)
    for info, shape, dtype in infos:
        assert all(np.isfinite(v) for v in info.values()), info
        assert tuple(shape) == (15, n) and dtype == torch.float32
    sd = torch.load(os.path.join(str(tmp_path), "c", "c_0", "net.p"))
    assert tuple(sd["action_out.weight"].shape) == (2 * n, 32)
    net = a2c_amd.FCModel(list(CC.STATE_SHAPE), n, h_size=32, is_discrete=False)
    net.load_state_dict(sd)
    net2 = copy.deepcopy(net).cuda()
    x = CC.model_input(1, "FCModel", 3, 32)[0].cuda()
    with torch.no_grad():
        a, b = net.cuda()(x), net2(x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0]) and torch.equal(a[1][1], b[1][1])
