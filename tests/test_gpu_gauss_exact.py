"""The per-sample Gaussian log-likelihood loss (hyps["gauss_loss"] = "exact") on the MI355X:
a2c_gauss_nll_fwd_bwd against a float64 autograd statement written here with torch.distributions.Normal (log_prob and
entropy summed over the action dims; independent of the kernel's closed forms), its shares, its argument checks, one
update_model against a float64 restatement of the two nets, the captured and the dispatcher paths, and a one-state bandit
that the reference loss cannot learn."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import a2c_amd
from a2c_amd import ops
from a2c_amd._lib import A2CKernelError
from a2c_amd.updater import Updater
import cont_cases as CC

pytestmark = pytest.mark.gpu
PI_C, VAL_C, ENT_C = 1.0, 0.5, 0.01
BLOCK_CAP = 1024          # the launch's grid cap (workgroups of 256 rows; include/a2c_mi355x.h): above 256 x this, a second trip


# ------------------------------------------------------------------------------------------------- the yardstick
def exact_loss(mu, raw, v, acts, advs, rets, norm, pi_coef, val_coef, entr_coef):
    """the loss in the dtype of its arguments: -pi_coef mean(w logp) + val_coef mean((V - R)^2) - entr_coef mean(H), logp and
    H of a diagonal Gaussian with sigma = softplus(raw) + 1e-4 -> (Loss, Pi_Loss, ValLoss, Entropy)"""
    dist = torch.distributions.Normal(mu, F.softplus(raw) + 1e-4)
    w = advs
    if norm:
        w = (w - w.mean()) / (w.std() + 1e-6)
    pi_loss = -pi_coef * (w * dist.log_prob(acts).sum(-1)).mean()
    val_loss = val_coef * ((v - rets) ** 2).mean()
    entr = entr_coef * dist.entropy().sum(-1).mean()
    return pi_loss + val_loss - entr, pi_loss, val_loss, entr


def heads_loss(heads, acts, advs, rets, n, norm, dtype=torch.float64):
    """exact_loss on heads rows [mu | raw | value | ...] -> (Pi_Loss, ValLoss, Entropy, d Loss / d heads[:, :2n + 1])"""
    h = heads[:, :2 * n + 1].to(dtype).clone().requires_grad_(True)
    loss, pi, vl, en = exact_loss(h[:, :n], h[:, n:2 * n], h[:, 2 * n], acts.to(dtype), advs.to(dtype), rets.to(dtype), norm,
                                  PI_C, VAL_C, ENT_C)
    loss.backward()
    return float(pi.detach()), float(vl.detach()), float(en.detach()), h.grad.double()


def rand_heads(N, n, seed, pad=0):
    """heads rows (N, 2n + 1 + pad) like _rand_heads of test_gpu_continuous.py: N(0, 1.5^2) with raw picks in every regime
    of the softplus (identity above 20, exactly 20) and of sigma (tiny, small, ordinary)"""
    g = torch.Generator().manual_seed(seed)
    heads = torch.randn(N, 2 * n + 1 + pad, generator=g) * 1.5
    raw = heads[:, n:2 * n]
    picks = torch.tensor([25.0, 20.0, 20.5, -9.0, -12.0, -3.4, 0.0])
    m = torch.rand(N, n, generator=g) < 0.3
    raw[m] = picks[torch.randint(0, len(picks), (int(m.sum()),), generator=g)]
    return heads


def kernel_inputs(N, n, on_policy, seed, zero_mean=False):
    heads = rand_heads(N, n, seed, pad=2)
    g = torch.Generator().manual_seed(seed * 7 + n)
    if on_policy:       # a = mu + sigma eps
        acts = heads[:, :n] + (F.softplus(heads[:, n:2 * n]) + 1e-4) * torch.randn(N, n, generator=g)
    else:
        acts = torch.randn(N, n, generator=g) * 1.3
    advs, rets = torch.randn(N, generator=g), torch.randn(N, generator=g)
    if zero_mean:       # x and -x: the mean is exactly 0 in any precision and any order
        advs = torch.cat([advs[:N // 2], -advs[:N // 2]])
    return heads, acts, advs, rets


def run_kernel(hd, ad, av, rt, n, norm, n_global=None, adv_sums=None, lo=0, hi=None):
    """one launch on rows lo:hi of device inputs, every argument strided: heads wider than 2n + 1 (the value column's stride
    is the row's), actions in a wider buffer, dheads with a guard column behind dV"""
    N = hd.shape[0]
    hi = N if hi is None else hi
    n_global = N if n_global is None else n_global
    stats = torch.zeros(8, dtype=torch.float64, device="cuda")
    if norm and adv_sums is None:
        adv_sums = stats[0:2]
        ops.moments(av, adv_sums)
    acts = torch.zeros(N, n + 1, device="cuda")
    acts[:, :n] = ad
    dh = torch.zeros(N, 2 * n + 2, device="cuda")
    ops.gauss_nll_fwd_bwd(hd[lo:hi, :2 * n], hd[lo:hi, 2 * n], acts[lo:hi, :n], av[lo:hi], rt[lo:hi],
                          adv_sums if norm else None, n_global, n, PI_C, VAL_C, ENT_C, dh[lo:hi, :2 * n], dh[lo:hi, 2 * n],
                          stats[2:5])
    torch.cuda.synchronize()
    return stats[2:5].clone(), dh


def grad_bound_ratio(got, want, n):
    """max over the entries of |err| / (1e-5 * (max |g| of that row's [dmu | draw]) + 1e-4 * |g|); dV (a column of another
    scale) against its own magnitude"""
    got, want = got.double(), want.double()
    err = (got - want).abs()
    pol = slice(0, 2 * n)
    bound = 1e-5 * want[:, pol].abs().max(dim=1, keepdim=True).values + 1e-4 * want[:, pol].abs()
    r_pol = float((err[:, pol] / bound.clamp_min(1e-300)).max())
    bv = (1e-5 + 1e-4) * want[:, 2 * n].abs()
    r_val = float((err[:, 2 * n] / bv.clamp_min(1e-300)).max())
    return max(r_pol, r_val)


def scalars(sums, N):
    """Updater._finish_host's reading of the three sums"""
    s = sums.cpu().numpy()
    return PI_C * -(s[0] / N), VAL_C * s[1] / N, -ENT_C * s[2] / N


def _close(name, got, want, atol, rtol):
    assert abs(got - want) <= atol + rtol * abs(want), (name, got, want)


# ------------------------------------------------------------------------------------------------------ 1. kernel
KERNEL_CASES = [  # N, n, norm_advs, on-policy actions, advantages of mean exactly 0
    (1, 1, False, True, False),
    (255, 1, True, False, False),
    (257, 32, False, True, False),
    (1000, 3, True, True, False),
    (77, 6, True, False, False),
    (5000, 2, True, True, False),
    (300, 64, False, True, False),
    (256 * BLOCK_CAP + 77, 1, True, True, False),       # the grid-stride loop's second trip
    (300, 1, False, False, True),
]


@pytest.mark.parametrize("N,n,norm,on_policy,zero_mean", KERNEL_CASES)
def test_kernel_matches_fp64_autograd(N, n, norm, on_policy, zero_mean):
    heads, acts, advs, rets = kernel_inputs(N, n, on_policy, 300 + N % 1000 + n, zero_mean)
    if zero_mean:
        assert float(advs.double().sum()) == 0.0
    pi, vl, en, grad = heads_loss(heads, acts, advs, rets, n, norm)
    hd, ad, av, rt = heads.cuda(), acts.cuda(), advs.cuda(), rets.cuda()
    (s0, d0), (s1, d1) = (run_kernel(hd, ad, av, rt, n, norm) for _ in range(2))
    assert torch.equal(s0, s1) and torch.equal(d0, d1)          # no atomics: two runs agree bit for bit
    assert torch.count_nonzero(d0[:, 2 * n + 1]) == 0           # the guard column
    got_pi, got_vl, got_en = scalars(s0, N)
    ratio = grad_bound_ratio(d0[:, :2 * n + 1].cpu(), grad, n)
    print(f"N={N} n={n}: Pi_Loss {got_pi!r} / {pi!r}  ValLoss {got_vl!r} / {vl!r}  Entropy {got_en!r} / {en!r}  "
          f"gradient error / bound {ratio:.4f}")
    _close("Pi_Loss", got_pi, pi, 1e-5, 1e-5)
    _close("ValLoss", got_vl, vl, 1e-5, 1e-5)
    _close("Entropy", got_en, en, 1e-6, 1e-5)
    assert ratio <= 1.0, ratio


# ------------------------------------------------------------------------------------------------------ 2. shares
def test_two_shares_equal_the_one_shot_run():
    N, n1, n = 1000, 400, 3
    heads, acts, advs, rets = kernel_inputs(N, n, True, 77)
    hd, ad, av, rt = heads.cuda(), acts.cuda(), advs.cuda(), rets.cuda()
    asum = torch.zeros(2, dtype=torch.float64, device="cuda")
    ops.moments(av, asum)
    s_all, d_all = run_kernel(hd, ad, av, rt, n, True, adv_sums=asum)
    s_a, d_a = run_kernel(hd, ad, av, rt, n, True, n_global=N, adv_sums=asum, lo=0, hi=n1)
    s_b, d_b = run_kernel(hd, ad, av, rt, n, True, n_global=N, adv_sums=asum, lo=n1, hi=N)
    assert torch.equal(d_a[:n1], d_all[:n1]) and torch.equal(d_b[n1:], d_all[n1:])
    assert torch.count_nonzero(d_a[n1:]) == 0 and torch.count_nonzero(d_b[:n1]) == 0
    np.testing.assert_allclose((s_a + s_b).cpu().numpy(), s_all.cpu().numpy(), rtol=1e-12, atol=0)


# --------------------------------------------------------------------------------------------------- 3. arguments
def test_argument_checks_leave_the_outputs_untouched():
    N, n = 64, 3
    heads, acts, advs, rets = kernel_inputs(N, n, True, 5)
    hd, ad, av, rt = heads.cuda(), acts.cuda(), advs.cuda(), rets.cuda()
    dh = torch.full((N, 2 * n + 1), 7.0, device="cuda")
    sums = torch.full((3,), 5.0, dtype=torch.float64, device="cuda")

    def call(n_arg, heads_rows=hd[:, :2 * n], rows=N):
        ops.gauss_nll_fwd_bwd(heads_rows[:rows], hd[:rows, 2 * n], ad[:rows], av[:rows], rt[:rows], None, N, n_arg, PI_C, VAL_C,
                              ENT_C, dh[:rows, :2 * n], dh[:rows, 2 * n], sums)
    wide = torch.zeros(N, 200, device="cuda")
    for bad in (lambda: call(0), lambda: call(65, heads_rows=wide),
                lambda: call(n, heads_rows=hd[:, :2 * n - 1].contiguous())):      # n = 0, 65; ld_heads < 2n
        with pytest.raises(A2CKernelError):
            bad()
    st = ops.stream()
    scratch = ops.reduce_scratch(hd.device, st)
    rc = ops.lib().a2c_gauss_nll_fwd_bwd(hd.data_ptr(), hd.stride(0), hd[:, 2 * n].data_ptr(), hd.stride(0), ad.data_ptr(), n,
                                         av.data_ptr(), rt.data_ptr(), None, N, N, n, PI_C, VAL_C, ENT_C, None, 2 * n + 1,
                                         dh[:, 2 * n].data_ptr(), 2 * n + 1, sums.data_ptr(), scratch.data_ptr(), st)
    with pytest.raises(A2CKernelError):         # a null output
        ops.check(rc, "a2c_gauss_nll_fwd_bwd")
    torch.cuda.synchronize()
    assert bool((dh == 7.0).all()) and bool((sums == 5.0).all())
    call(n, rows=0)                             # n_local = 0 zeroes the sums and writes nothing else
    torch.cuda.synchronize()
    assert bool((sums == 0.0).all()) and bool((dh == 7.0).all())


# ------------------------------------------------------------------------------------- 4. one update against fp64
def net64(kind, sd, dtype):
    """FCModel / GRUFCModel restated from the state-dict keys in `dtype`: -> (parameters by name, rows(x, h) -> (heads
    rows [mu | raw | value], new h or None))"""
    P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    h = P["base.2.weight"].shape[0]

    def lin(x, name):
        return x @ P[name + ".weight"].T + P[name + ".bias"]

    def rows(x, hs=None):
        f = lin(torch.relu(lin(x.reshape(x.shape[0], -1), "base.0")), "base.2")
        if kind == "GRUFCModel":
            Wx, Wh, b = P["gru.W_x"], P["gru.W_h"], P["gru.b"]
            z = torch.sigmoid(f @ Wx[0] + hs @ Wh[0] + b[0])
            r = torch.sigmoid(f @ Wx[1] + hs @ Wh[1] + b[1])
            c = torch.tanh(f @ Wx[2] + (r * hs) @ Wh[2] + b[2])
            f = z * hs + (1 - z) * c
        ln = F.layer_norm(f, (h,), P["value_out.0.weight"], P["value_out.0.bias"])
        v = lin(lin(ln, "value_out.1"), "value_out.2")
        return torch.cat([lin(f, "action_out"), v], dim=1), (f if kind == "GRUFCModel" else None)
    return P, rows


def scan64(x, dones, g):
    """y[i] = x[i] + g * (1 - dones[i]) * y[i + 1] (utils.discount), in float64"""
    y, run = torch.zeros_like(x), 0.0
    for i in range(x.numel() - 1, -1, -1):
        run = float(x[i]) + g * (0.0 if float(dones[i]) == 1.0 else run)
        y[i] = run
    return y


def update64(kind, sd, n, hyps, D, use_bptt, dtype=torch.float64):
    """one A2C update with the exact loss, restated: forward (flat, recurrent-flat or stepped over time with the done
    reset), exact_loss, clip_grad_norm_, torch.optim -> (info, parameters by name)"""
    P, rows = net64(kind, sd, dtype)
    R_, T = hyps["n_rollouts"], hyps["n_tsteps"]
    S, dn = D["states"].to(dtype), D["dones"].double()
    advs = scan64(D["deltas"].double(), dn, hyps["gamma"] * hyps["lambda_"]).to(dtype)
    rets = scan64(D["rewards"].double(), dn, hyps["gamma"]).to(dtype)
    if use_bptt:
        hs = D["h_states"].to(dtype).view(R_, T, -1)[:, 0]
        keep = (1 - dn.to(dtype)).view(R_, T, 1)
        outs = []
        for t in range(T):
            o, hs = rows(S.view(R_, T, *S.shape[1:])[:, t], hs)
            hs = hs * keep[:, t]
            outs.append(o)
        heads = torch.stack(outs, dim=1).reshape(R_ * T, -1)
    else:
        heads = rows(S, D["h_states"].to(dtype) if kind == "GRUFCModel" else None)[0]
    loss, pi, vl, en = exact_loss(heads[:, :n], heads[:, n:2 * n], heads[:, 2 * n], D["actions"].to(dtype), advs, rets,
                                  hyps["norm_advs"], hyps["pi_coef"], hyps["val_coef"], hyps["entr_coef"])
    loss.backward()
    params = list(P.values())
    gnorm = torch.nn.utils.clip_grad_norm_(params, hyps["max_norm"])
    getattr(torch.optim, hyps["optim_type"])(params, lr=hyps["lr"]).step()
    info = {"Loss": float(loss.detach()), "Pi_Loss": float(pi.detach()), "ValLoss": float(vl.detach()), "Entropy": float(en.detach()),
            "GradNorm": float(gnorm)}
    return info, {k: v.detach().double() for k, v in P.items()}


UPDATE_R, UPDATE_T, UPDATE_H = 6, 5, 16
# n = 3 has no entry in cont_cases.UPDATE_RAW_BIAS: the first three of its six-wide row
RAW_BIAS = {**CC.UPDATE_RAW_BIAS, 3: CC.UPDATE_RAW_BIAS[6][:3]}
UPDATE_CASES = [  # name, kind, n, use_bptt, optim, lr, norm_advs, seed
    ("fc_n1_sgd", "FCModel", 1, False, "SGD", 0.1, True, 2100),
    ("fc_n3_sgd", "FCModel", 3, False, "SGD", 0.1, False, 2110),
    ("fc_n3_rms", "FCModel", 3, False, "RMSprop", 1e-4, True, 2110),
    ("grufc_n2_sgd", "GRUFCModel", 2, False, "SGD", 0.1, True, 2120),
    ("grufc_bptt_n1_sgd", "GRUFCModel", 1, True, "SGD", 0.1, False, 2130),
]


def update_case(case):
    """-> (state dict, hyps, host shared data) of one case"""
    name, kind, n, use_bptt, opt, lr, norm, seed = case
    sd = CC.state_dict(kind, n, UPDATE_H, RAW_BIAS[n])
    hyps = CC.cont_hyps(n_tsteps=UPDATE_T, n_rollouts=UPDATE_R, optim_type=opt, lr=lr, norm_advs=norm, use_bptt=use_bptt,
                        h_size=UPDATE_H, gauss_loss="exact")
    D = CC.synth_shared(n, UPDATE_H, UPDATE_R, UPDATE_T, seed=seed, recurrent=kind == "GRUFCModel")
    return sd, hyps, D


def info_bound_ratio(info, want):
    return max(abs(info[k] - want[k]) / (1e-5 + 3e-5 * abs(want[k])) for k in want)


def param_bound_ratio(got, want):
    return max(float(((got[k].double() - want[k]).abs() / (1e-5 + 1e-5 * want[k].abs())).max()) for k in want)


def _gpu_net(kind, n, sd):
    net = getattr(a2c_amd, kind)(list(CC.STATE_SHAPE), n, h_size=UPDATE_H, is_discrete=False)
    net.load_state_dict(sd)
    return net.cuda()


@pytest.mark.parametrize("case", UPDATE_CASES, ids=[c[0] for c in UPDATE_CASES])
def test_update_matches_fp64_restatement(case):
    name, kind, n, use_bptt = case[:4]
    sd, hyps, D = update_case(case)
    want_info, want_P = update64(kind, sd, n, hyps, D, use_bptt)
    net = _gpu_net(kind, n, sd)
    upd = Updater(net, hyps)
    info = upd.update_model({k: v.cuda() for k, v in D.items()})
    assert "gsums" not in upd._bufs
    got_P = {k: p.detach().cpu() for k, p in net.named_parameters()}
    assert sorted(got_P) == sorted(want_P)
    ri, rp = info_bound_ratio(info, want_info), param_bound_ratio(got_P, want_P)
    moved = max(float((want_P[k] - sd[k].double()).abs().max()) for k in want_P)
    print(f"{name}: info error / bound {ri:.4f}, parameter error / bound {rp:.4f}, largest parameter step {moved:.3e}", info)
    assert moved > 1e-4         # the update moved the parameters by far more than the bound
    assert ri <= 1.0, (info, want_info)
    assert rp <= 1.0


# ------------------------------------------------------------------------------------------- 5. graph, dispatcher
def _exact_update_case(kind, n, R_, T, opt, norm, seed, use_bptt=False, h=16):
    net = getattr(a2c_amd, kind)(list(CC.STATE_SHAPE), n, h_size=h, is_discrete=False)
    net.load_state_dict(CC.state_dict(kind, n, h, CC.UPDATE_RAW_BIAS[n]))
    net = net.cuda()
    hyps = CC.cont_hyps(n_tsteps=T, n_rollouts=R_, optim_type=opt, norm_advs=norm, use_bptt=use_bptt, h_size=h,
                        gauss_loss="exact")
    D = {k: v.cuda() for k, v in CC.synth_shared(n, h, R_, T, seed=seed, recurrent=net.is_recurrent).items()}
    return net, Updater(net, hyps), D


@pytest.mark.parametrize("kind,use_bptt", [("FCModel", False), ("GRUFCModel", True)])
def test_graphed_update_equals_eager(kind, use_bptt):
    def run(graphed):
        net, upd, D = _exact_update_case(kind, 2, 3, 4, "RMSprop", True, 1600, use_bptt=use_bptt)
        infos = [upd.update_model(D)]
        if graphed:
            rep = upd.capture_update(D)
            assert len(rep.graphs) == 1
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
        net, upd, D = _exact_update_case("FCModel", 6, 3, 5, "RMSprop", True, 1700)
        info = upd.update_model(D)
        return info, torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    i0, p0 = run()
    monkeypatch.setenv("A2C_TORCH_OPS", "1")
    if not os.path.exists(os.path.join(os.path.dirname(ops.__file__), "liba2c_torch_ops.so")):
        pytest.fail("liba2c_torch_ops.so was not built")
    cnt =lambda d, k: sum(v for name, v in d.items() if name.endswith(k))
    before = dict(ops.torch_abi().stats["by_name"])
    i1, p1 = run()
    after = ops.torch_abi().stats["by_name"]
    assert hasattr(torch.ops.a2c_mi355x, "abi_gauss_nll_fwd_bwd")
    assert cnt(after, "gauss_nll_fwd_bwd") > cnt(before, "gauss_nll_fwd_bwd"), after
    for k in ("gauss_loss_sums", "gauss_loss_fwd_bwd"):         # the reference pair is not launched
        assert cnt(after, k) == cnt(before, k), (k, after)
    assert torch.equal(p0, p1) and i0 == i1


# ------------------------------------------------------------------------------------------------ 6. it learns
BANDIT_ROWS, BANDIT_UPDATES, BANDIT_TARGET = 256, 60, 1.5


def bandit_hyps(**kw):
    return CC.cont_hyps(n_tsteps=BANDIT_ROWS, n_rollouts=1, n_frame_stack=1, gamma=0.0, lambda_=0.0, optim_type="RMSprop", lr=1e-3,
                        max_norm=0.5, norm_advs=True, entr_coef=0.001, val_coef=0.5, h_size=32, **kw)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 2])
def test_bandit_mu_moves_to_the_rewarded_action(n, seed):
    """One state (a constant observation of 0.25), reward -sum((a - 1.5)^2), gamma 0: 60 updates of 256 sampled rows must
    bring |mu - 1.5| to at most a quarter of where it started.  The reference loss (and so a build that ignores the key)
    leaves it above 0.9 of it: its mu gradient is one batch-wide factor, a sum of zero-mean weights under norm_advs."""
    torch.manual_seed(seed)
    net = a2c_amd.FCModel([1, 1, 8], n, h_size=32, is_discrete=False).cuda()
    upd = Updater(net, bandit_hyps(gauss_loss="exact"))
    N = BANDIT_ROWS
    states = torch.full((N, 1, 1, 8), 0.25, device="cuda")
    dones = torch.zeros(N, device="cuda")
    dones[-1] = 1.0
    eps = torch.randn(BANDIT_UPDATES, N, n, generator=torch.Generator().manual_seed(100 + seed)).cuda()
    acts = torch.zeros(N, n, device="cuda")

    def miss():
        with torch.no_grad():
            return float((net(states)[1][0] - BANDIT_TARGET).abs().max())
    start = miss()
    for k in range(BANDIT_UPDATES):
        with torch.no_grad():
            v = net(states)[0].view(-1).clone()
        ops.gauss_head(net._heads("pub", N)[1], n, N, eps=eps[k], actions_ptr=acts.data_ptr(), act_ld=n)
        r = -((acts - BANDIT_TARGET) ** 2).sum(dim=1)
        info = upd.update_model(dict(states=states, actions=acts, rewards=r, dones=dones, deltas=r - v))
    end = miss()
    print(f"n={n} seed={seed}: |mu - 1.5| {start:.4f} -> {end:.4f} ({end / start:.4f} of the start)", info)
    assert all(np.isfinite(x) for x in info.values()), info
    assert end <= 0.25 * start, (start, end)
