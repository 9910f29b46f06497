"""-m gpu: the capturable Adam family (Adam, AdamW, Adamax, NAdam, RAdam, ASGD with ``capturable=True``): the step count and
the step-dependent scalars live in a device block (a2c_optim_advance), the step kernel reads them there
(a2c_clip_step_dev), and Updater.capture_update replays the pair.

1 the block's scalars against the host formulas after every advance, 2 the device-scalar step kernels against fp64 by the
criterion of test_gpu_optimizers, 3 graphed == eager, 4 whole updates against the oracle, 5 the published state,
6 checkpoints within and across the two modes and from the reference, 7 the mode is fixed, 8 the torch-ops boundary and a
world-2 sharded capture.
"""
import copy
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from oracle import a2c_oracle as O  # noqa: E402
from cases import CHECKPOINT_CASES, base_hyps, synth_shared  # noqa: E402
from test_gpu_kernels import close  # noqa: E402
from test_gpu_models import make_net  # noqa: E402
import test_gpu_optimizers as T  # noqa: E402

DEV = "cuda"
SIX = ("Adam", "AdamW", "Adamax", "NAdam", "RAdam", "ASGD")


def _f32(x):
    return float(np.float32(x))


def _ulp_diff(a, b):
    """distance of two python floats in fp32 ulps (both are rounded to fp32 first)"""
    ia, ib = (int(np.float32(v).view(np.int32)) for v in (a, b))
    ia, ib = (-(i & 0x7FFFFFFF) if i < 0 else i for i in (ia, ib))
    return abs(ia - ib)


def _torch_group(name, **group):
    """torch's own default param_group of the class (lr 1e-3), updated"""
    g = dict(getattr(torch.optim, name)([torch.zeros(1, requires_grad=True)], lr=1e-3).defaults)
    g.update(group)
    return g


def _advance(ops, name, blk, grp):
    b1, b2 = grp.get("betas", (0.0, 0.0))
    ops.optim_advance(ops.OPTIM_KINDS[name], blk, grp["lr"], b1, b2, grp.get("eps", 0.0), grp.get("weight_decay", 0.0),
                      grp.get("momentum_decay", 0.0), grp.get("lambd", 0.0), grp.get("alpha", 0.0), grp.get("t0", 0.0))


# ------------------------------------------------------------------ 1: the scalars
def _host_derived(name, grp, s, before, after):
    """the derived fields a2c_optim_advance writes at step s, by the formulas of the host launchers (a2c_clip_<name>) in
    python doubles.  before / after: the block's running fp32 state before and after this advance (the launchers take
    NAdam's mu_product and ASGD's eta / mu as arguments too)"""
    lr = grp["lr"]
    b1, b2 = grp.get("betas", (0.0, 0.0))
    out = dict(lr=_f32(lr), omb1=_f32(1.0 - b1), beta2=_f32(b2), omb2=_f32(1.0 - b2), eps=_f32(grp.get("eps", 0.0)))
    if name in ("Adam", "AdamW"):
        bc1, bc2 = 1.0 - b1 ** s, 1.0 - b2 ** s
        out.update(step_size=_f32(lr / bc1), bc2_sqrt=_f32(math.sqrt(bc2)), decay=_f32(1.0 - lr * grp["weight_decay"]))
    elif name == "Adamax":
        out.update(neg_clr=_f32(-(lr / (1.0 - b1 ** s))))
    elif name == "NAdam":
        md, mp_ = grp["momentum_decay"], after["mu_product"]
        mu = b1 * (1.0 - 0.5 * 0.96 ** (s * md))
        mu_next = b1 * (1.0 - 0.5 * 0.96 ** ((s + 1.0) * md))
        out.update(bc2=_f32(1.0 - b2 ** s), c_grad=_f32(-lr * (1.0 - mu) / (1.0 - mp_)),
                   c_avg=_f32((-lr * mu_next) / (1.0 - mp_ * mu_next)))
    elif name == "RAdam":
        bc1, bc2 = 1.0 - b1 ** s, 1.0 - b2 ** s
        rho_inf = 2.0 / (1.0 - b2) - 1.0
        rho_t = rho_inf - 2.0 * s * b2 ** s / bc2
        rectify = rho_t > 5.0
        rect = ((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t)) ** 0.5 if rectify else 0.0
        out.update(bc1=_f32(bc1), bc2_sqrt=_f32(bc2 ** 0.5), rect=_f32(rect), rectify=int(rectify))
    else:
        eta, mu = before["eta"], before["mu"]
        out.update(decay=_f32(1.0 - grp["lambd"] * eta), neg_eta=_f32(-eta), mu_used=_f32(mu), mu_is_one=int(_f32(mu) == 1.0))
    return out


SCALAR_CASES = {"Adam": ("Adam", {}), "AdamW": ("AdamW", {}), "Adamax": ("Adamax", {}), "NAdam": ("NAdam", {}),
                "RAdam": ("RAdam", {}), "RAdam-beta2_0.8": ("RAdam", dict(betas=(0.9, 0.8))),
                "ASGD": ("ASGD", {}), "ASGD-t0_0": ("ASGD", dict(t0=0.0))}


@pytest.mark.parametrize("start", [0, 999, 100000])
@pytest.mark.parametrize("case", list(SCALAR_CASES))
def test_advance_scalars_equal_the_host_formulas(case, start):
    """64 advances from a fresh block and from loaded steps 999 and 100 000.  The step count and the integer flags are exact.
    Every fp32 scalar is within one fp32 ulp of the host formula: both sides round doubles that differ by a few double
    ulps at most (host libm's pow against the device's), which moves the fp32 rounding by one ulp or not at all.  The
    derived scalars are formed from the block's own running state (the launchers take it as an argument); the running
    state itself is compared with the host chain (optim.nadam_mu_product / asgd_eta_mu): one ulp per step taken for the
    product, one ulp for eta / mu, which do not depend on their previous values."""
    from a2c_amd import ops
    from a2c_amd.optim import asgd_eta_mu, nadam_mu_product
    name, group = SCALAR_CASES[case]
    grp = _torch_group(name, **group)
    run = dict(mu_product=1.0, eta=_f32(grp["lr"]), mu=1.0)          # the host chain
    if name == "NAdam":
        for s in range(1, start + 1):
            run["mu_product"] = nadam_mu_product(run["mu_product"], s, grp["betas"][0], grp["momentum_decay"])
    if name == "ASGD" and start:
        run["eta"], run["mu"] = asgd_eta_mu(start, grp["lr"], grp["lambd"], grp["alpha"], grp["t0"])
    blk = ops.optim_block_new(DEV)
    ops.optim_block_set(blk, start, run["mu_product"], run["eta"], run["mu"])
    before = ops.optim_block_read(blk)
    assert before["step"] == start and all(before[k] == run[k] for k in run)
    n_scalars = n_bitwise = worst = 0
    flags = set()
    for s in range(start + 1, start + 65):
        _advance(ops, name, blk, grp)
        after = ops.optim_block_read(blk)
        assert after["step"] == s
        if name == "NAdam":
            run["mu_product"] = nadam_mu_product(run["mu_product"], s, grp["betas"][0], grp["momentum_decay"])
            assert _ulp_diff(after["mu_product"], run["mu_product"]) <= s - start, (case, s)
        else:
            assert after["mu_product"] == before["mu_product"]
        if name == "ASGD":
            run["eta"], run["mu"] = asgd_eta_mu(s, grp["lr"], grp["lambd"], grp["alpha"], grp["t0"])
            assert _ulp_diff(after["eta"], run["eta"]) <= 1 and _ulp_diff(after["mu"], run["mu"]) <= 1, (case, s)
        else:
            assert (after["eta"], after["mu"]) == (before["eta"], before["mu"])
        for k, want in _host_derived(name, grp, float(s), before, after).items():
            if k in ("rectify", "mu_is_one"):
                assert after[k] == want, (case, s, k)
                flags.add((k, want))
                continue
            d = _ulp_diff(after[k], want)
            assert d <= 1, (case, s, k, after[k], want)
            n_scalars += 1
            n_bitwise += d != 0
            worst = max(worst, d)
        before = after
    print(f"{case} from step {start}: {n_bitwise} of {n_scalars} scalars differ bitwise from the host's (worst {worst} ulp)")
    if name == "RAdam":                # the run from 0 crosses rho_t = 5; the loaded ones are past it
        assert flags == ({("rectify", 0), ("rectify", 1)} if start == 0 else {("rectify", 1)})
    if case == "ASGD":                 # t0 = 1e6: mu stays 1 up to step 1e6
        assert flags == {("mu_is_one", 1)}
    if case == "ASGD-t0_0":            # mu = 1 / step: one only where the previous step was 0 or 1
        assert flags == ({("mu_is_one", 0), ("mu_is_one", 1)} if start == 0 else {("mu_is_one", 0)})


# ------------------------------------------------------------------ 2: the step kernel against fp64
class _DevLaunch:
    """test_gpu_optimizers._launch through the device-scalar path: one block per parameter array, started at the step
    before the first launch it sees (ASGD: with the eta / mu torch stored before it), advanced once per launch"""

    def __init__(self):
        self.blocks = {}

    def __call__(self, ops, name, grp, tstate, p, g, s, sumsq, norm, step, max_norm=0.5):
        blk = self.blocks.get(p.data_ptr())
        if blk is None:
            assert step == 1 or name != "NAdam"
            blk = self.blocks[p.data_ptr()] = ops.optim_block_new(p.device)
            ops.optim_block_set(blk, step - 1, 1.0, tstate.get("eta", 0.0), tstate.get("mu", 1.0))
        _advance(ops, name, blk, grp)
        ops.clip_step_dev(ops.OPTIM_KINDS[name], p, g, s[0], s[1] if len(s) > 1 else None, sumsq, max_norm, blk, norm)
        assert ops.optim_block_read(blk)["step"] == step


@pytest.fixture
def dev_launch(monkeypatch):
    monkeypatch.setattr(T, "_launch", _DevLaunch())


def _run_trio(t, name, n, grads, tag, ulp_distance=False):
    """the steps of one _Trio and, after each, the project's criterion on the parameters and every state array
    (test_gpu_optimizers._criterion: worst <= 2 ref + one fp32 ulp, worst = max |kernel - fp64|, ref = max |torch fp32 -
    fp64|, the ulp that of max |fp64|) and the sentinels.  ulp_distance: also the per-element form of
    test_clip_kernel_vs_torch_optim, max ulp distance of the kernel's parameters from torch's fp32 ones <= 2 x that of
    torch's fp32 from its fp64 ones + 1.  That form is asserted where that test asserts it, on parameters of size 1: the
    ulp distance of an element is its error over ITS OWN size, so where parameters cancel to near zero (p0 of size 0 is
    the accumulated update) both maxima are set by whichever element happens to lie closest to zero and their ratio is
    not bounded by anything -- measured on an MI355X for NAdam at p0 = 0: 524 288 against 244 684 ulp, with the criterion
    above met at every step, and the host-scalar kernel (a2c_clip_nadam) gives the same two figures there.  It is printed
    for every run."""
    worst = ref = 0
    for k, g in enumerate(grads, 1):
        t.step(g)
        t.check(f"{tag} step {k}")
        worst = max(worst, T._ulps(t.pd, t.p32.detach()[:n]))
        ref = max(ref, T._ulps(t.p32.detach(), t.p64.detach().float()))
    print(f"{name} {tag}: max param distance {worst} ulp, torch fp32 from fp64: {ref} ulp")
    t.report(f"{name} {tag}")
    if ulp_distance:
        assert worst <= 2 * ref + 1, (name, tag, worst, ref)


@pytest.mark.parametrize("name", SIX)
def test_device_scalar_step_vs_torch_optim(name, dev_launch):
    """test_clip_kernel_vs_torch_optim's second run (torch stepping on the kernel's clipped gradient) through the device path"""
    n = 10007
    t = T._Trio(name, T.rnd((n,), 220))
    grads = [T.rnd((n,), 221 + k) * (0.02 if k == 2 else 0.001) for k in range(1, T.STEPS + 1)]      # step 2 clips
    _run_trio(t, name, n, grads, "hashed p0 of size 1", ulp_distance=True)


@pytest.mark.parametrize("scale", list(T.SCALES))
@pytest.mark.parametrize("name", SIX)
def test_device_scalar_step_against_fp64(name, scale, dev_launch):
    n = 10007
    t = T._Trio(name, T._rand(n, 300) * T.SCALES[scale])
    _run_trio(t, name, n, [T._grad(name, n, k, 310) for k in range(1, T.STEPS + 1)], f"p0 of size {scale}")
    if name == "RAdam":
        assert 1 < T._radam_first_rectified(t.grp["betas"]) <= T.STEPS
    if name == "ASGD":
        assert float(t.state()["mu"]) != 1.0             # t0 = 2: the averaging branch ran


@pytest.mark.parametrize("n", [1, 3, 4, 5])
@pytest.mark.parametrize("name", SIX)
def test_device_scalar_step_small_sizes(name, n, dev_launch):
    t = T._Trio(name, T._rand(n, 400) * 1e-3, pool=4096)
    _run_trio(t, name, n, [T._grad(name, n, k, 410) for k in range(1, T.STEPS + 1)], f"n {n}")


@pytest.mark.parametrize("name", SIX)
def test_device_scalar_step_three_grid_stride_passes(name, dev_launch):
    n = T.BIG_N
    t = T._Trio(name, T._rand(n, 500) * 1e-3)
    if name == "RAdam":                                       # starts at step 5 so that the 3 steps cross rho_t = 5
        t.warm([T._grad(name, n, k, 505) for k in range(1, 6)])
        assert t.step_no < T._radam_first_rectified(t.grp["betas"]) <= t.step_no + 3
    _run_trio(t, name, n, [T._grad(name, n, k, 510) for k in range(1, 4)], f"n {n}")


def test_device_scalar_entry_points_validate():
    from a2c_amd import ops
    lib = ops.lib()
    blk = ops.optim_block_new(DEV)
    a = torch.zeros(64, device=DEV)
    sumsq = torch.zeros(1, dtype=torch.float64, device=DEV)
    P = lambda t, off=0: t.data_ptr() + off                  # noqa: E731
    adv = lambda kind, b: lib.a2c_optim_advance(kind, b, 1e-3, .9, .999, 1e-8, 0., 0., 0., 0., 0., ops.stream())   # noqa: E731
    assert adv(0, None) == -1 and adv(0, P(blk, 8)) == -1 and adv(6, P(blk)) == -1 and adv(-1, P(blk)) == -1
    step = lambda kind, p, g, sa, sb, n, ss, b: lib.a2c_clip_step_dev(kind, p, g, sa, sb, n, ss, 0.5, b, None, ops.stream())  # noqa: E731
    ok = (P(a), P(a, 64), P(a, 128), P(a, 192))
    assert step(0, *ok, 0, P(sumsq), P(blk)) == 0 and step(0, None, None, None, None, 0, P(sumsq), P(blk)) == 0
    assert step(0, *ok, 4, P(sumsq), None) == -1 and step(0, *ok, 4, P(sumsq), P(blk, 4)) == -1
    assert step(9, *ok, 4, P(sumsq), P(blk)) == -1 and step(0, *ok, -1, P(sumsq), P(blk)) == -1
    assert step(0, *ok, 4, None, P(blk)) == -1
    for k in range(4):
        bad = list(ok)
        bad[k] = None
        assert step(0, *bad, 4, P(sumsq), P(blk)) == -1
        assert step(5, *bad, 4, P(sumsq), P(blk)) == (0 if k == 3 else -1)        # ASGD has one state array
        bad[k] = ok[k] + 4
        assert step(0, *bad, 4, P(sumsq), P(blk)) == -1
    torch.cuda.synchronize()
    assert ops.optim_block_read(blk)["step"] == 0            # nothing was advanced, the one valid ASGD launch read zeros


# ------------------------------------------------------------------ 3: graphed == eager, both capturable
def _case(name, case, **extra):
    kind, ss, A, h, R_, T_, bptt = case
    net = make_net(kind, ss, A, h)
    hyps = base_hyps(n_tsteps=T_, n_rollouts=R_, optim_type=name, use_bptt=bptt, h_size=h, optim_capturable=True, **extra)
    return net, hyps


def _block(upd):
    from a2c_amd import ops
    return ops.optim_block_read(upd.optim._block)


@pytest.mark.parametrize("how", ["replay", "replay_async"])
@pytest.mark.parametrize("name", SIX)
def test_capturable_graphed_equals_eager(name, how):
    from a2c_amd.updater import Updater

    def run(graphed):
        net, hyps = _case(name, T.A3C)
        upd = Updater(net, hyps)
        assert upd.optim.capture_safe and upd.optim.param_groups[0]["capturable"] is True
        _, D = T._data(T.A3C, 0, net)
        infos = [upd.update_model(D)]
        if graphed:
            rep = upd.capture_update(D)
            infos += [rep.replay() if how == "replay" else upd.collect(rep.replay_async()) for _ in range(3)]
        else:
            infos += [upd.update_model(D) for _ in range(3)]
        torch.cuda.synchronize()
        return (infos, net._arena.params.clone(), {k: v.clone() for k, v in upd.optim._flat.items()}, upd.optim._steps,
                _block(upd))
    ie, pe, se, ne, be = run(False)
    ig, pg, sg, ng, bg = run(True)
    assert torch.equal(pe, pg)
    assert se.keys() == sg.keys() and all(torch.equal(se[k], sg[k]) for k in se)
    assert ie == ig and ne == ng == 4
    assert be == bg and bg["step"] == 4
    assert len({i["Loss"] for i in ig}) == 4                 # the replays did step


# ------------------------------------------------------------------ 4: against the oracle
def _tol(name, lr):
    # Adam belongs with test_gpu_optimizers.NORMALISING by the reasoning written there (the Adam family's first steps move a
    # weight by about lr whatever |g| is); it is missing from that list only because that file tests the other optimisers
    return 2 * lr if name == "Adam" else T._param_tol(name, lr)


@pytest.mark.parametrize("case", [T.A3C, T.FC], ids=["A3CModel", "FCModel"])
@pytest.mark.parametrize("name", SIX)
def test_capturable_updates_vs_oracle(name, case):
    from a2c_amd.updater import Updater
    kind, ss, A, h = case[:4]
    net, hyps = _case(name, case)
    upd = Updater(net, hyps)
    onet = O.OracleNet(kind, ss, A, h)
    oupd = O.OracleUpdater(onet, hyps)
    assert type(oupd.optim).__name__ == name and upd.optim._capturable
    dev = 0.0
    for u in range(3):
        D, Dd = T._data(case, u, net)
        info, oinfo = upd.update_model(Dd), oupd.update_model(D)
        dev = max(dev, T._check_update(f"{name} u{u}", net, onet, info, oinfo, _tol(name, hyps["lr"])))
    print(f"capturable {name} {kind}: max parameter deviation from the oracle {dev:.3e}")


# ------------------------------------------------------------------ 5: the published state
@pytest.mark.parametrize("name", SIX)
def test_capturable_state_dict_is_torchs(name):
    from a2c_amd.optim import asgd_eta_mu, nadam_mu_product
    from a2c_amd.updater import Updater
    net, hyps = _case(name, T.A3C)
    upd = Updater(net, hyps)
    _, D = T._data(T.A3C, 0, net)
    upd.update_model(D)
    rep = upd.capture_update(D)
    for _ in range(3):
        rep.replay()
    sd = upd.optim.state_dict()
    # torch's own capturable optimiser of the class, one step on the device
    p = torch.zeros(4, device=DEV, requires_grad=True)
    topt = getattr(torch.optim, name)([p], lr=hyps["lr"], capturable=True)
    p.grad = torch.ones(4, device=DEV)
    topt.step()
    ref = topt.state_dict()
    assert set(sd["param_groups"][0]) == set(ref["param_groups"][0])
    assert {k: v for k, v in sd["param_groups"][0].items() if k != "params"} == \
        {k: v for k, v in ref["param_groups"][0].items() if k != "params"}
    assert sd["param_groups"][0]["capturable"] is True
    grp = sd["param_groups"][0]
    want = {}
    if name == "NAdam":
        want["mu_product"] = 1.0
        for s in range(1, 5):
            want["mu_product"] = nadam_mu_product(want["mu_product"], s, grp["betas"][0], grp["momentum_decay"])
    if name == "ASGD":
        want["eta"], want["mu"] = asgd_eta_mu(4, grp["lr"], grp["lambd"], grp["alpha"], grp["t0"])
    assert len(sd["state"]) > 0
    for i, st in sd["state"].items():
        assert set(st) == set(ref["state"][0]), i
        step = st["step"]
        assert step.is_cuda and step.dtype == torch.float32 and step.dim() == 0 and float(step) == 4.0
        for k, w in want.items():
            assert st[k].is_cuda and st[k].dtype == torch.float32 and st[k].dim() == 0
            assert st[k].device == ref["state"][0][k].device
            assert _ulp_diff(float(st[k]), w) <= 4, (name, k)           # one ulp per step taken
    assert upd.optim._steps == 4


# ------------------------------------------------------------------ 6: checkpoints
GROUPS = {"ASGD": dict(t0=4.0)}          # update 5 is the last to store mu = 1, 7 the first to average (as STRADDLE)


def _fc_updater(name, capturable, group=None):
    from a2c_amd.updater import Updater
    kind, ss, A, h, R_, T_, _ = T.FC
    upd = Updater(make_net(kind, ss, A, h), base_hyps(n_tsteps=T_, n_rollouts=R_, optim_type=name, h_size=h,
                                                      optim_capturable=capturable))
    upd.optim.param_groups[0].update(group or {})
    assert upd.optim._capturable == capturable
    return upd


def _steps(upd, ks):
    out = []
    for k in ks:
        upd.net._arena.train_grads().copy_(T._host_grad(upd.net._arena, k))
        upd.optim.step(max_norm=0.5)
        torch.cuda.synchronize()
        out.append((upd.net._arena.params.clone(), {s: v.clone() for s, v in upd.optim._flat.items()},
                    T._host_scalars(upd.optim)))
    return out


@pytest.mark.parametrize("name", SIX)
def test_capturable_checkpoint_continues_bit_identically(name):
    a = _fc_updater(name, True, GROUPS.get(name))
    _steps(a, range(1, 6))
    sd, params = copy.deepcopy(a.optim.state_dict()), a.net._arena.params.clone()
    want = _steps(a, range(6, 9))
    b = _fc_updater(name, True)
    b.net._arena.params.copy_(params)
    b.net.mark_dirty()
    b.optim.load_state_dict(sd)
    assert b.optim._steps == 5 and _block(b)["step"] == 5
    assert all(b.optim.param_groups[0][k] == v for k, v in a.optim.param_groups[0].items() if k != "params")
    got = _steps(b, range(6, 9))
    for k, ((pa, fa, ha), (pb, fb, hb)) in enumerate(zip(want, got), 6):
        assert torch.equal(pa, pb), (name, k)
        assert fa.keys() == fb.keys() and all(torch.equal(fa[s], fb[s]) for s in fa), (name, k)
        assert ha == hb and ha["step"] == {float(k)}, (name, k)
    assert _block(a) == _block(b)


@pytest.mark.parametrize("direction", ["capturable_to_host", "host_to_capturable"])
@pytest.mark.parametrize("name", SIX)
def test_checkpoint_crosses_the_modes(name, direction):
    """five updates in one mode, the state_dict into a fresh optimiser of the other mode, three more: the step count is
    equal, the running scalars within the bound of the scalar test (one ulp per step for mu_product, one ulp for eta / mu),
    and the parameters meet the fp64 criterion against the uninterrupted torch runs"""
    first = direction == "capturable_to_host"
    group = GROUPS.get(name, {})
    a = _fc_updater(name, first, group)
    ar = a.net._arena
    p0 = ar.train_params().detach().cpu().clone()
    p32, p64 = p0.clone().requires_grad_(True), p0.double().requires_grad_(True)
    lr = a.optim.param_groups[0]["lr"]
    opt32, opt64 = (getattr(torch.optim, name)([p], lr=lr) for p in (p32, p64))
    for o in (opt32, opt64):
        o.param_groups[0].update(group)

    def torch_steps(ks):
        for k in ks:
            p32.grad = T._host_grad(ar, k).clone()
            torch.nn.utils.clip_grad_norm_([p32], 0.5)
            opt32.step()
            p64.grad = p32.grad.double()
            opt64.step()

    _steps(a, range(1, 6))
    torch_steps(range(1, 6))
    T._criterion(f"{name} {direction} update 5", ar.train_params(), p32, p64)
    sd, params = copy.deepcopy(a.optim.state_dict()), ar.params.clone()
    assert sd["param_groups"][0]["capturable"] is first
    b = _fc_updater(name, not first)
    b.net._arena.params.copy_(params)
    b.net.mark_dirty()
    b.optim.load_state_dict(sd)
    assert b.optim.param_groups[0]["capturable"] is (not first)       # the object keeps its own mode
    assert b.optim._steps == a.optim._steps == 5
    ha, hb = T._host_scalars(a.optim), T._host_scalars(b.optim)
    assert ha["step"] == hb["step"] == {5.0}
    for k in a.optim._scalars:
        (va,), (vb,) = ha[k], hb[k]
        assert va == vb, (name, k)                                     # a loaded value is stored as it is
    got = _steps(b, range(6, 9))
    torch_steps(range(6, 9))
    T._criterion(f"{name} {direction} update 8", b.net._arena.train_params(), p32, p64)
    want = opt32.state[p32]
    assert got[-1][2]["step"] == {8.0} and b.optim._steps == 8
    for k in b.optim._scalars:
        (v,) = got[-1][2][k]
        assert _ulp_diff(v, float(want[k])) <= (8 if k == "mu_product" else 1), (name, k)


def test_reference_checkpoint_loads_into_capturable_adam(golden):
    """tests/golden/g7_grufc_adam_{net,optim}.p (written by the reference, capturable=False in its group) into a
    capturable Adam: the next update lands on the reference's next weights, at test_resume_from_reference_written_
    checkpoint's tolerances"""
    import a2c_amd
    from a2c_amd.updater import Updater
    g = golden["g7_checkpoint"]
    case = [c for c in CHECKPOINT_CASES if c[0] == "grufc_adam"][0]
    name, kind, ss, A, h, R_, T_, opt, use_bptt = case
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    net = getattr(a2c_amd.models, kind)(list(ss), A, h_size=h, bnorm=False)
    net.load_state_dict(torch.load(os.path.join(gdir, f"g7_{name}_net.p"), weights_only=False))
    hyps = base_hyps(n_tsteps=T_, n_rollouts=R_, optim_type=opt, use_bptt=use_bptt, h_size=h, optim_capturable=True)
    upd = Updater(net, hyps)
    upd.optim.load_state_dict(torch.load(os.path.join(gdir, f"g7_{name}_optim.p"), weights_only=False))
    assert upd.optim._capturable and upd.optim.param_groups[0]["capturable"] is True
    assert upd.optim._steps == 1 and _block(upd)["step"] == 1
    D = synth_shared(kind, ss, A, h, R_, T_, seed=920, recurrent=net.is_recurrent)
    D = {k: (v.to(DEV) if k != "actions" else v) for k, v in D.items()}
    info = upd.update_model(D)
    for k in ("Loss", "Pi_Loss", "ValLoss", "Entropy"):
        assert info[k] == pytest.approx(float(g[f"{name}_{k}"]), rel=3e-5, abs=2e-6), k
    assert info["GradNorm"] == pytest.approx(float(g[f"{name}_GradNorm"]), rel=3e-4)
    for n, p in net.named_parameters():
        close(f"param {n}", p.detach(), g[f"{name}_param_{n}"], 3e-5, 1e-5)
    assert _block(upd)["step"] == 2


# ------------------------------------------------------------------ 7: the mode is fixed, the default is unchanged
@pytest.mark.parametrize("name", SIX)
def test_mode_is_fixed_at_construction(name):
    from a2c_amd import optim as fused_optim
    cap, host = _fc_updater(name, True), _fc_updater(name, False)
    assert cap.optim.capture_safe and not host.optim.capture_safe
    assert host.optim.param_groups[0]["capturable"] is False and host.optim._block is None
    assert isinstance(cap.optim, fused_optim.OPTIMIZERS[name])
    for upd, flipped in ((cap, False), (host, True)):
        upd.net._arena.train_grads().copy_(T._host_grad(upd.net._arena, 1))
        upd.optim.step(max_norm=0.5)
        before = upd.net._arena.params.clone()
        upd.optim.param_groups[0]["capturable"] = flipped
        with pytest.raises(ValueError, match="capturable"):
            upd.optim.step(max_norm=0.5)
        torch.cuda.synchronize()
        assert torch.equal(upd.net._arena.params, before) and upd.optim._steps == 1


def test_optim_capturable_leaves_the_capture_safe_optimisers_alone():
    from a2c_amd import optim as fused_optim
    from a2c_amd.updater import Updater
    res = []
    for flag in (False, True):
        kind, ss, A, h, R_, T_, _ = T.FC
        net = make_net(kind, ss, A, h)
        upd = Updater(net, base_hyps(n_tsteps=T_, n_rollouts=R_, optim_type="RMSprop", h_size=h, optim_capturable=flag))
        assert upd.optim.param_groups[0]["capturable"] is False and upd.optim._block is None and upd.optim.capture_safe
        _, D = T._data(T.FC, 0, net)
        info = upd.update_model(D)
        torch.cuda.synchronize()
        res.append((info, net._arena.params.clone(), upd.optim._flat["square_avg"].clone(),
                    {k: v for k, v in upd.optim.param_groups[0].items() if k != "params"}))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert res[0][3] == res[1][3]
    with pytest.raises(TypeError):
        fused_optim.RMSprop(net, capturable=True)
    with pytest.raises(TypeError):
        fused_optim.Adagrad(net, capturable=True)


# ------------------------------------------------------------------ 8: the torch-ops boundary and a sharded capture
@pytest.mark.parametrize("name", ["Adam", "NAdam"])
def test_capturable_torch_ops_path_is_bit_identical(name, monkeypatch):
    from a2c_amd import ops
    from a2c_amd.updater import Updater
    res = {}
    for mode in ("ctypes", "torch_ops"):
        if mode == "torch_ops":
            monkeypatch.setenv("A2C_TORCH_OPS", "1")
            ops.torch_abi().stats.update(torch_ops=0, ctypes=0, by_name={}, unresolved={})
        net, hyps = _case(name, T.FC)
        upd = Updater(net, hyps)
        _, D = T._data(T.FC, 0, net)
        infos = [dict(upd.update_model(D)), dict(upd.update_model(D))]
        torch.cuda.synchronize()
        res[mode] = (infos, net._arena.params.cpu().clone(), net._arena.grads.cpu().clone(),
                     {k: v.cpu().clone() for k, v in upd.optim._flat.items()}, _block(upd))
    monkeypatch.delenv("A2C_TORCH_OPS")
    st = ops.torch_abi().stats
    assert st["unresolved"] == {} and st["ctypes"] == 0, st
    assert st["by_name"].get("a2c_optim_advance", 0) == 2 and st["by_name"].get("a2c_clip_step_dev", 0) == 2, st
    (ia, pa, ga, sa, ba), (ib, pb, gb, sb, bb) = res["ctypes"], res["torch_ops"]
    assert ia == ib and torch.equal(pa, pb) and torch.equal(ga, gb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert ba == bb and ba["step"] == 2


def _sharded_adam_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", A2C_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "pytorch-a2c_amd"), os.path.join(root, "tests", "golden"),
                    os.path.join(root, "tests")]
    import torch.distributed as dist
    from a2c_amd import ops
    from a2c_amd.parallel import Shard
    from a2c_amd.updater import Updater
    from test_gpu_models import make_net
    from cases import base_hyps, synth_shared
    torch.cuda.set_device(0)
    kind, ss, A, h, R, T_ = "A3CModel", (4, 84, 84), 3, 256, 4, 6
    sh = Shard.from_env()
    lo, hi = sh.slot_range(R)
    out = {}
    for graphed in (False, True):              # both ranks take the same branch: the collectives stay paired
        net = make_net(kind, ss, A, h)
        upd = Updater(net, base_hyps(n_tsteps=T_, n_rollouts=hi - lo, optim_type="Adam", h_size=h, optim_capturable=True),
                      shard=sh)
        infos, Dl, g = [], None, None
        for u in range(4):
            D = synth_shared(kind, ss, A, h, R, T_, seed=700 + 10 * u, recurrent=False)
            new = {k: v[lo * T_:hi * T_].cuda() for k, v in D.items()}
            if Dl is None:
                Dl = new
            else:
                for k in Dl:                   # a captured update replays on the SAME buffers
                    Dl[k].copy_(new[k])
            if u == 0 or not graphed:
                infos.append(upd.update_model(Dl))
            else:
                if g is None:
                    g = upd.capture_update(Dl)
                infos.append(g.replay())
        torch.cuda.synchronize()
        out[graphed] = (infos, [p.detach().cpu().numpy() for p in net.parameters()], upd.optim._steps,
                        ops.optim_block_read(upd.optim._block)["step"], 0 if g is None else g.fallbacks)
    q.put((rank, out))
    dist.destroy_process_group()


def test_sharded_capturable_adam_graphed_equals_eager():
    """world 2 (gloo, both ranks on cuda:0), A3CModel, capturable Adam: one eager update, capture_update and three replays
    on new data, against the same four sharded updates run eagerly.  Each rank has its own block and advances alike."""
    from test_gpu_system import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sharded_adam_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, out in res:
        (ie, pe, ne, be, _), (ig, pg, ng, bg, fallbacks) = out[False], out[True]
        assert fallbacks == 0 and ne == ng == be == bg == 4
        assert ie == ig, rank
        assert all(np.array_equal(a, b) for a, b in zip(pe, pg)), rank
    for a, b in zip(res[0][1][True][1], res[1][1][True][1]):
        assert np.array_equal(a, b)
