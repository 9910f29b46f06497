"""-m gpu: the fused clip + step kernels of the torch.optim optimisers beyond RMSprop / Adam (a2c_clip_<name>), against
torch.optim on the CPU (the reference's own code path, _single_tensor_<name>) and, inside whole updates, against the
oracle's Updater, which builds its optimiser by name like the reference."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import a2c_oracle as O  # noqa: E402
from cases import base_hyps, synth_shared  # noqa: E402
from test_gpu_kernels import close, rnd  # noqa: E402
from test_gpu_models import make_net  # noqa: E402

DEV = "cuda"
NEW = ("SGD", "Adagrad", "Adadelta", "Rprop", "AdamW", "Adamax", "NAdam", "RAdam", "ASGD")
STATE = {"SGD": (), "Adagrad": ("sum",), "Adadelta": ("square_avg", "acc_delta"), "Rprop": ("prev", "step_size"),
         "AdamW": ("exp_avg", "exp_avg_sq"), "Adamax": ("exp_avg", "exp_inf"), "NAdam": ("exp_avg", "exp_avg_sq"),
         "RAdam": ("exp_avg", "exp_avg_sq"), "ASGD": ("ax",)}
CAPTURABLE = ("SGD", "Adagrad", "Adadelta", "Rprop")
# param groups loaded into both sides: Rprop's clamps and ASGD's t0 are reached within the 5 steps
GROUP = {"Rprop": dict(step_sizes=(5e-4, 1.3e-3)), "ASGD": dict(t0=2.0)}
LR = {"Adadelta": 1.0}


def _ulps(a, b):
    ia = a.detach().cpu().float().view(torch.int32).long()
    ib = b.detach().cpu().float().view(torch.int32).long()
    ia = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int((ia - ib).abs().max())


def _launch(ops, name, grp, tstate, p, g, s, sumsq, norm, step):
    lr = grp["lr"]
    if name == "SGD":
        ops.clip_sgd(p, g, sumsq, 0.5, lr, norm)
    elif name == "Adagrad":
        ops.clip_adagrad(p, g, s[0], sumsq, 0.5, lr, grp["lr_decay"], grp["eps"], step, norm)
    elif name == "Adadelta":
        ops.clip_adadelta(p, g, s[0], s[1], sumsq, 0.5, lr, grp["rho"], grp["eps"], norm)
    elif name == "Rprop":
        ops.clip_rprop(p, g, s[0], s[1], sumsq, 0.5, *grp["etas"], *grp["step_sizes"], norm)
    elif name == "AdamW":
        ops.clip_adamw(p, g, s[0], s[1], sumsq, 0.5, lr, *grp["betas"], grp["eps"], grp["weight_decay"], step, norm)
    elif name == "Adamax":
        ops.clip_adamax(p, g, s[0], s[1], sumsq, 0.5, lr, *grp["betas"], grp["eps"], step, norm)
    elif name == "NAdam":       # the kernel takes the product torch stored after this step
        ops.clip_nadam(p, g, s[0], s[1], sumsq, 0.5, lr, *grp["betas"], grp["eps"], grp["momentum_decay"], step,
                       float(tstate["mu_product"]), norm)
    elif name == "RAdam":
        ops.clip_radam(p, g, s[0], s[1], sumsq, 0.5, lr, *grp["betas"], grp["eps"], step, norm)
    elif name == "ASGD":        # ... and the eta / mu torch stored BEFORE this step
        ops.clip_asgd(p, g, s[0], sumsq, 0.5, grp["lambd"], tstate["eta"], tstate["mu"], norm)


@pytest.mark.parametrize("name", NEW)
def test_clip_kernel_vs_torch_optim(name):
    from a2c_amd import ops
    n = 10007                                        # float4 groups + a 3-element tail
    p0 = rnd((n,), 220)
    ref_p = p0.clone().requires_grad_(True)
    opt = getattr(torch.optim, name)([ref_p], lr=LR.get(name, 1e-3))
    opt.param_groups[0].update(GROUP.get(name, {}))
    grp = opt.param_groups[0]
    pd = torch.zeros(n + 1, device=DEV)[:n]
    pd.copy_(p0)
    gd = torch.zeros(n, device=DEV)
    s = [torch.zeros(n, device=DEV) for _ in STATE[name]]
    if name == "Rprop":
        s[1].fill_(grp["lr"])                        # torch fills step_size with lr at the first step
    sumsq = torch.zeros(1, dtype=torch.float64, device=DEV)
    norm = torch.zeros(1, device=DEV)
    half = torch.arange(n) % 2 == 1
    worst = 0
    for step in range(1, 6):
        g = rnd((n,), 221 + step) * (0.02 if step == 2 else 0.001)            # step 2 clips, the others do not
        if name == "Rprop":          # odd elements flip sign every step (etaminus, lower clamp), even ones keep it (upper)
            g = rnd((n,), 221).abs() * (0.02 if step == 2 else 0.001) * torch.where(half, torch.tensor(-1.0) ** step, 1.0)
        if name == "ASGD":           # this step uses the eta / mu the previous one stored (fp32 lr and 1 at first)
            st0 = opt.state[ref_p]
            pre = (float(st0["eta"]), float(st0["mu"])) if st0 else (float(np.float32(grp["lr"])), 1.0)
        ref_p.grad = g.clone()
        tn = torch.nn.utils.clip_grad_norm_([ref_p], 0.5)
        opt.step()
        tstate = dict(opt.state[ref_p])
        if name == "ASGD":
            tstate.update(eta=pre[0], mu=pre[1])
        gd.copy_(g)
        ops.gradnorm_sq(gd, sumsq)
        _launch(ops, name, grp, tstate, pd, gd, s, sumsq, norm, step)
        torch.cuda.synchronize()
        assert norm.item() == pytest.approx(float(tn), rel=2e-6)
        close(f"{name} clipped grad step {step}", gd, ref_p.grad, 1e-10, 2e-6)
        close(f"{name} params step {step}", pd, ref_p.detach(), 2e-7, 1e-6)
        for k, sd in zip(STATE[name], s):
            want = opt.state[ref_p][k]
            # (exp_avg's lerp cancels: torch's vectorised CPU path rounds it differently, a few ulp of the array's scale)
            close(f"{name} {k} step {step}", sd, want, 2e-6 * float(want.abs().max()) + 1e-30, 4e-6)
        worst = max(worst, _ulps(pd, ref_p))
    if name == "Rprop":
        ss = opt.state[ref_p]["step_size"]
        assert float(ss.min()) == pytest.approx(5e-4) and float(ss.max()) == pytest.approx(1.3e-3)   # both clamps
    if name == "ASGD":
        assert float(opt.state[ref_p]["mu"]) != 1.0
    print(f"{name}: max param difference {worst} ulp over 5 steps")


# ------------------------------------------------------------------ whole updates against the oracle
A3C = ("A3CModel", (4, 84, 84), 3, 256, 4, 8, False)
FC = ("FCModel", (4, 4), 2, 200, 4, 32, False)
GRU = ("GRUModel", (4, 84, 84), 3, 256, 3, 6, True)
UPD = [(n, A3C) for n in NEW] + [(n, FC) for n in NEW] + [("AdamW", GRU), ("Adagrad", GRU)]
# Rules that normalise the gradient's size (Adagrad's and the Adam family's first steps, Adamax) move a weight by
# about lr whatever |g| is, so where fp32 noise flips the sign of a near-zero gradient the two sides differ by up to
# 2 lr after one step.  Rprop moves every weight by its step size (up to lr * 1.2^2 by the third update) in the
# gradient's sign: the same flip costs twice that per update, over three updates.
NORMALISING = ("Adagrad", "AdamW", "Adamax", "NAdam")


def _param_tol(name, lr):
    if name == "Rprop":
        return 6 * 1.44 * lr
    if name in NORMALISING:
        return 2 * lr
    return 3e-5


def _case(name, case, seed=700):
    kind, ss, A, h, R_, T, bptt = case
    net = make_net(kind, ss, A, h)
    hyps = base_hyps(n_tsteps=T, n_rollouts=R_, optim_type=name, use_bptt=bptt, h_size=h)
    return net, hyps


def _data(case, u, net):
    kind, ss, A, h, R_, T, _ = case
    D = synth_shared(kind, ss, A, h, R_, T, seed=700 + 10 * u, recurrent=net.is_recurrent)
    return D, {k: v.to(DEV) for k, v in D.items()}


def _check_update(tag, net, onet, info, oinfo, tol):
    for k in ("Loss", "Pi_Loss", "ValLoss", "Entropy"):
        assert info[k] == pytest.approx(float(oinfo[k]), rel=3e-5, abs=2e-6), (tag, k, info[k], float(oinfo[k]))
    dev = 0.0
    for (n, p), (_, q) in zip(net.named_parameters(), onet.named_parameters()):
        close(f"{tag} param {n}", p.detach(), q.detach(), tol, 1e-5)
        dev = max(dev, float((p.detach().cpu() - q.detach()).abs().max()))
    return dev


@pytest.mark.parametrize("name,case", UPD, ids=[f"{n}-{c[0]}" for n, c in UPD])
def test_updates_vs_oracle(name, case):
    from a2c_amd.updater import Updater
    kind, ss, A, h = case[:4]
    net, hyps = _case(name, case)
    upd = Updater(net, hyps)
    onet = O.OracleNet(kind, ss, A, h)
    oupd = O.OracleUpdater(onet, hyps)
    assert type(oupd.optim).__name__ == name
    dev = 0.0
    for u in range(3):
        D, Dd = _data(case, u, net)
        info, oinfo = upd.update_model(Dd), oupd.update_model(D)
        dev = max(dev, _check_update(f"{name} u{u}", net, onet, info, oinfo, _param_tol(name, hyps["lr"])))
    print(f"{name} {kind}: max parameter deviation from the oracle {dev:.3e}")


def _cpu_sd(sd):
    return {"state": {k: {s: (v.cpu() if torch.is_tensor(v) else v) for s, v in st.items()} for k, st in sd["state"].items()},
            "param_groups": sd["param_groups"]}


@pytest.mark.parametrize("name", NEW)
def test_state_dict_matches_torch_and_round_trips(name):
    from a2c_amd.updater import Updater
    case = A3C
    kind, ss, A, h = case[:4]
    net, hyps = _case(name, case)
    upd = Updater(net, hyps)
    onet = O.OracleNet(kind, ss, A, h)
    oupd = O.OracleUpdater(onet, hyps)
    D, Dd = _data(case, 0, net)
    upd.update_model(Dd)
    oupd.update_model(D)
    sd, ref = upd.optim.state_dict(), oupd.optim.state_dict()
    assert sd["param_groups"] == ref["param_groups"]
    assert set(sd["state"]) == set(ref["state"])          # Adagrad: every parameter (emb_bnorm too); SGD: none
    if name == "SGD":
        assert sd["state"] == {}
    if name == "Adagrad":
        assert len(sd["state"]) == len(list(net.parameters()))
    for k in ref["state"]:
        assert set(sd["state"][k]) == set(ref["state"][k]), k
        for s, want in ref["state"][k].items():
            got = sd["state"][k][s]
            assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (k, s)
            if s == "step":
                assert float(got) == float(want)
            elif want.dim() == 0:
                assert float(got) == float(want), (k, s)
            else:
                close(f"{name} state {k}.{s}", got, want, 1e-9 + 1e-3 * float(want.abs().max()), 2e-3)
    # ours loads into torch.optim itself
    getattr(torch.optim, name)(O.OracleNet(kind, ss, A, h).parameters(), lr=hyps["lr"]).load_state_dict(_cpu_sd(sd))
    # new_lr (training.py's decay_lr) keeps the state
    before = _cpu_sd(upd.optim.state_dict())
    upd.new_lr(hyps["lr"])
    after = _cpu_sd(upd.optim.state_dict())
    assert set(after["state"]) == set(before["state"])
    for k in before["state"]:
        for s in before["state"][k]:
            assert torch.equal(torch.as_tensor(after["state"][k][s]), torch.as_tensor(before["state"][k][s])), (k, s)
    # the oracle's torch-written dict loads into a fresh updater on the oracle's weights; the next update lands on the
    # oracle's next weights
    net2 = make_net(kind, ss, A, h)
    with torch.no_grad():
        for (_, p), (_, q) in zip(net2.named_parameters(), onet.named_parameters()):
            p.copy_(q)
    net2.mark_dirty()
    upd2 = Updater(net2, hyps)
    upd2.optim.load_state_dict(ref)
    assert upd2.optim._steps == (0 if name == "SGD" else 1)
    D, Dd = _data(case, 1, net2)
    info, oinfo = upd2.update_model(Dd), oupd.update_model(D)
    _check_update(f"{name} resumed", net2, onet, info, oinfo, _param_tol(name, hyps["lr"]))


def test_loaded_settings_the_kernels_lack_are_refused():
    from a2c_amd.updater import Updater
    kind, ss, A, h, R_, T, _ = FC
    for name, bad in (("SGD", dict(momentum=0.9)), ("SGD", dict(nesterov=True)), ("Adagrad", dict(weight_decay=0.1)),
                      ("AdamW", dict(amsgrad=True)), ("NAdam", dict(decoupled_weight_decay=True)),
                      ("Rprop", dict(maximize=True)), ("ASGD", dict(weight_decay=1e-3))):
        upd = Updater(make_net(kind, ss, A, h), base_hyps(n_tsteps=T, n_rollouts=R_, optim_type=name, h_size=h))
        sd = upd.optim.state_dict()
        sd["param_groups"][0].update(bad)
        with pytest.raises(ValueError, match=list(bad)[0]):
            upd.optim.load_state_dict(sd)


# ------------------------------------------------------------------ hipGraph capture
@pytest.mark.parametrize("name", CAPTURABLE)
def test_capture_replays_equal_eager(name):
    def run(graphed):
        net, hyps = _case(name, A3C)
        from a2c_amd.updater import Updater
        upd = Updater(net, hyps)
        _, D = _data(A3C, 0, net)
        infos = [upd.update_model(D)]
        if graphed:
            rep = upd.capture_update(D)
            infos += [rep(), rep(), rep()]
        else:
            infos += [upd.update_model(D) for _ in range(3)]
        torch.cuda.synchronize()
        return infos, net._arena.params.clone(), {k: v.clone() for k, v in upd.optim._flat.items()}, upd.optim._steps
    ie, pe, se, ne = run(False)
    ig, pg, sg, ng = run(True)
    assert torch.equal(pe, pg)
    assert se.keys() == sg.keys() and all(torch.equal(se[k], sg[k]) for k in se)
    assert ie == ig and ne == ng == 4


@pytest.mark.parametrize("name", [n for n in NEW if n not in CAPTURABLE])
def test_capture_refuses_step_dependent_optimisers(name):
    from a2c_amd.updater import Updater
    net, hyps = _case(name, A3C)
    upd = Updater(net, hyps)
    _, D = _data(A3C, 0, net)
    upd.update_model(D)
    with pytest.raises(RuntimeError, match="step count"):
        upd.capture_update(D)


def test_adagrad_with_lr_decay_is_not_capture_safe():
    from a2c_amd.updater import Updater
    net, hyps = _case("Adagrad", FC)
    upd = Updater(net, hyps)
    assert upd.optim.capture_safe
    upd.optim.param_groups[0]["lr_decay"] = 0.01
    assert not upd.optim.capture_safe


# ------------------------------------------------------------------ torch-ops routing
@pytest.mark.parametrize("name", NEW)
def test_torch_ops_path_is_bit_identical(name, monkeypatch):
    from a2c_amd import ops
    from a2c_amd.updater import Updater
    res = {}
    for mode in ("ctypes", "torch_ops"):
        if mode == "torch_ops":
            monkeypatch.setenv("A2C_TORCH_OPS", "1")
            ops.torch_abi().stats.update(torch_ops=0, ctypes=0, by_name={}, unresolved={})
        net, hyps = _case(name, FC)
        upd = Updater(net, hyps)
        _, D = _data(FC, 0, net)
        info = upd.update_model(D)
        torch.cuda.synchronize()
        res[mode] = (dict(info), net._arena.params.cpu().clone(), net._arena.grads.cpu().clone(),
                     {k: v.cpu().clone() for k, v in upd.optim._flat.items()})
    monkeypatch.delenv("A2C_TORCH_OPS")
    st = ops.torch_abi().stats
    assert st["unresolved"] == {} and st["ctypes"] == 0, st
    assert st["by_name"].get(f"a2c_clip_{name.lower()}", 0) == 1, st
    (ia, pa, ga, sa), (ib, pb, gb, sb) = res["ctypes"], res["torch_ops"]
    assert ia == ib and torch.equal(pa, pb) and torch.equal(ga, gb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


# ------------------------------------------------------------------ training loop
def test_train_two_epochs_adamw(tmp_path):
    from a2c_amd.training import train
    hyps = dict(exp_name="w", main_path=str(tmp_path), model="A3CModel", env_type="FakeBreakout", n_envs=3, n_rollouts=3,
                n_tsteps=5, max_tsteps=1e9, action_size=3, seed=1, n_test_eps=1, optim_type="AdamW", env_pool="serial")
    best = train(None, hyps, verbose=False, env_fn=lambda j: O.FakeEnv(env_id=j, rew_period=3, done_period=7),
                 max_epochs=2)
    assert np.isfinite(best)
    osd = torch.load(os.path.join(str(tmp_path), "w", "w_0", "optim.p"))
    assert osd["param_groups"][0]["weight_decay"] == 0.01 and osd["param_groups"][0]["decoupled_weight_decay"]
    assert {float(st["step"]) for st in osd["state"].values()} == {2.0}
    net = O.OracleNet("A3CModel", (4, 84, 84), 3, 256)
    torch.optim.AdamW(net.parameters(), lr=1e-3).load_state_dict(_cpu_sd(osd))
