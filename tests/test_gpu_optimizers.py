"""-m gpu: the fused clip + step kernels of the torch.optim optimisers (a2c_clip_<name>), against torch.optim on the CPU
(the reference's own code path, _single_tensor_<name>) and, inside whole updates, against the oracle's Updater, which
builds its optimiser by name like the reference.

Kernel level, all eleven rules: every step is also compared with torch.optim run in fp64 on the same clipped gradients,
and the kernel may be at most twice as far from it as torch's own fp32 run plus one fp32 ulp (`_criterion`), from
parameters of size 1, 1e-3 and 0, over 12 steps (RAdam across its rectification threshold, Adagrad with lr_decay, ASGD
before and past t0), at n from 1 to three grid-stride passes with a sentinel behind every array, on gradients with
signed zeros, underflowing squares and large entries, and at the edges of the clip coefficient.  The host classes'
step-dependent scalars run 40 updates against torch and through checkpoints that straddle a branch.
Worst e_k / e_t of the parameters measured on an MI355X over all of these: RMSprop 1.24, Adam 1.13, SGD 1.44, Adagrad 1.28,
Adadelta 1.30, Rprop 1.00, AdamW 1.05, Adamax 1.25, NAdam 1.18, RAdam 1.30, ASGD 1.74; of a state array 1.99 (Adagrad's sum).
"""
import copy
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
# rule -> (state arrays, lr of the kernel-level tests, param-group settings loaded into both sides: Rprop's clamps and
# ASGD's t0 are reached within a few steps)
ALL = {
    "RMSprop": (("square_avg",), 1e-3, {}),
    "Adam": (("exp_avg", "exp_avg_sq"), 1e-3, {}),
    "SGD": ((), 1e-3, {}),
    "Adagrad": (("sum",), 1e-3, {}),
    "Adadelta": (("square_avg", "acc_delta"), 1.0, {}),
    "Rprop": (("prev", "step_size"), 1e-3, dict(step_sizes=(5e-4, 1.3e-3))),
    "AdamW": (("exp_avg", "exp_avg_sq"), 1e-3, {}),
    "Adamax": (("exp_avg", "exp_inf"), 1e-3, {}),
    "NAdam": (("exp_avg", "exp_avg_sq"), 1e-3, {}),
    "RAdam": (("exp_avg", "exp_avg_sq"), 1e-3, {}),
    "ASGD": (("ax",), 1e-3, dict(t0=2.0)),
}
NEW = tuple(n for n in ALL if n not in ("RMSprop", "Adam"))
CAPTURABLE = ("SGD", "Adagrad", "Adadelta", "Rprop")
STEPS = 12
PAD, SENTINEL = 64, 0x4B1D5EED       # floats allocated behind every device array, and the bit pattern they must keep


def _bits(t):
    return t.detach().cpu().float().clone().view(torch.int32)


def _ulps(a, b):
    ia, ib = _bits(a).long(), _bits(b).long()
    ia = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int((ia - ib).abs().max())


def _rand(n, seed):
    """uniform in (-1, 1) at full fp32 resolution (cases.hashf has 256 distinct values)"""
    return torch.from_numpy(np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32))


def _with_norm(g, norm):
    """g rescaled in fp64 to the given 2-norm"""
    return (g.double() * (norm / float(g.double().norm()))).float()


def _grad(name, n, k, seed):
    """the gradient of the k-th step of a run: norm 0.05, under max_norm = 0.5 (coefficient exactly 1), but norm 2 at
    steps 2 and 9 (clipped)"""
    g = _rand(n, seed + k)
    if name == "Rprop":     # odd elements flip sign every step (etaminus, lower clamp), even ones keep it (etaplus, upper)
        g = _rand(n, seed).abs() * torch.where(torch.arange(n) % 2 == 1, torch.tensor(-1.0) ** k, 1.0)
    return _with_norm(g, 2.0 if k in (2, 9) else 0.05)


def _radam_first_rectified(betas):
    """the first step with rho_t > 5 (torch/optim/radam.py), from the group's betas"""
    beta2 = betas[1]
    rho_inf = 2 / (1 - beta2) - 1
    assert rho_inf > 5
    s = 1
    while rho_inf - 2 * s * beta2 ** s / (1 - beta2 ** s) <= 5.0:
        s += 1
    return s


def _launch(ops, name, grp, tstate, p, g, s, sumsq, norm, step, max_norm=0.5):
    lr = grp["lr"]
    if name == "RMSprop":
        ops.clip_rmsprop(p, g, s[0], sumsq, max_norm, lr, grp["alpha"], grp["eps"], norm)
    elif name == "Adam":
        ops.clip_adam(p, g, s[0], s[1], sumsq, max_norm, lr, *grp["betas"], grp["eps"], step, norm)
    elif name == "SGD":
        ops.clip_sgd(p, g, sumsq, max_norm, lr, norm)
    elif name == "Adagrad":
        ops.clip_adagrad(p, g, s[0], sumsq, max_norm, lr, grp["lr_decay"], grp["eps"], step, norm)
    elif name == "Adadelta":
        ops.clip_adadelta(p, g, s[0], s[1], sumsq, max_norm, lr, grp["rho"], grp["eps"], norm)
    elif name == "Rprop":
        ops.clip_rprop(p, g, s[0], s[1], sumsq, max_norm, *grp["etas"], *grp["step_sizes"], norm)
    elif name == "AdamW":
        ops.clip_adamw(p, g, s[0], s[1], sumsq, max_norm, lr, *grp["betas"], grp["eps"], grp["weight_decay"], step, norm)
    elif name == "Adamax":
        ops.clip_adamax(p, g, s[0], s[1], sumsq, max_norm, lr, *grp["betas"], grp["eps"], step, norm)
    elif name == "NAdam":       # the kernel takes the product torch stored after this step
        ops.clip_nadam(p, g, s[0], s[1], sumsq, max_norm, lr, *grp["betas"], grp["eps"], grp["momentum_decay"], step,
                       float(tstate["mu_product"]), norm)
    elif name == "RAdam":
        ops.clip_radam(p, g, s[0], s[1], sumsq, max_norm, lr, *grp["betas"], grp["eps"], step, norm)
    elif name == "ASGD":        # ... and the eta / mu torch stored BEFORE this step
        ops.clip_asgd(p, g, s[0], sumsq, max_norm, grp["lambd"], tstate["eta"], tstate["mu"], norm)


def _criterion(tag, got, t32, t64, n=None):
    """e_k = max|kernel - fp64| <= 2 e_t + one fp32 ulp of max|fp64|, e_t = max|torch fp32 - fp64|: the kernel resolves
    the update as well as torch's own fp32 run does.  2, because torch's vectorised CPU kernels round some ops (lerp_
    is one fused multiply-add there) differently from the scalar order the functors follow.  n: `got` is the first n
    elements, e_t is over all of them (_Trio's pool).  -> e_k / e_t, None if e_t == 0"""
    t64 = t64.detach()
    n = t64.numel() if n is None else n
    e_k = float((got.detach().cpu().double() - t64[:n]).abs().max())
    e_t = float((t32.detach().double() - t64).abs().max())
    ulp = float(np.spacing(np.float32(t64[:n].abs().max())))
    assert e_k <= 2 * e_t + ulp, f"{tag}: e_k {e_k:.3e} > 2 * e_t {e_t:.3e} + ulp {ulp:.3e} (ratio {e_k / max(e_t, 1e-300):.3g})"
    return e_k / e_t if e_t > 0 else None


def _dev(n):
    buf = torch.empty(n + PAD, device=DEV)
    buf.view(torch.int32).fill_(SENTINEL)
    buf[:n] = 0
    return buf


class _Trio:
    """One rule three times over the same given gradients: the kernel, torch.optim in fp32 and torch.optim in fp64 fed
    the fp32 run's clipped gradients.  The gradients are inputs, not functions of the parameters, so the three do not
    drift apart.  Every device array has PAD sentinel floats behind it."""

    def __init__(self, name, p0, group=None, pool=0):
        """pool: elements behind the kernel's n that only the two torch runs step, from parameters and gradients of the
        same distribution and with the kernel's own clip coefficient.  e_t is taken over them too: at n = 1 the error of
        a single element of torch's fp32 run is often 0 by chance, and says nothing about how well fp32 resolves the step"""
        from a2c_amd import ops
        self.ops, self.name, self.n, self.pool = ops, name, p0.numel(), pool
        self.names, lr, grp = ALL[name]
        scale = float(p0.abs().max())
        self.p32 = torch.cat([p0, _rand(pool, 99) * scale]).requires_grad_(True)
        self.p64 = self.p32.detach().double().requires_grad_(True)
        self.opt32, self.opt64 = (getattr(torch.optim, name)([p], lr=lr) for p in (self.p32, self.p64))
        for o in (self.opt32, self.opt64):
            o.param_groups[0].update(grp if group is None else group)
        self.grp = self.opt32.param_groups[0]
        self.buf = {k: _dev(self.n) for k in ("param", "grad") + self.names}
        self.pd, self.gd = self.buf["param"][:self.n], self.buf["grad"][:self.n]
        self.s = [self.buf[k][:self.n] for k in self.names]
        self.pd.copy_(p0)
        if name == "Rprop":
            self.s[1].fill_(self.grp["lr"])                  # torch fills step_size with lr at the first step
        self.sumsq = torch.zeros(1, dtype=torch.float64, device=DEV)
        self.norm = torch.zeros(1, device=DEV)
        self.step_no = 0
        self.worst = {}                                      # array -> worst e_k / e_t

    def state(self, wide=False):
        return self.opt64.state[self.p64] if wide else self.opt32.state[self.p32]

    def _torch_step(self, clipped):
        self.p32.grad = clipped.clone()
        self.opt32.step()
        self.p64.grad = clipped.double()
        self.opt64.step()
        if self.name == "NAdam":
            self.mu_product = float(self.state()["mu_product"])

    def warm(self, grads, max_norm=0.5):
        """steps taken by torch alone; the kernel's arrays then start from torch's fp32 ones"""
        for g in grads:
            self.step_no += 1
            self.tgrad = g.clone().requires_grad_(True)
            self.tgrad.grad = g.clone()
            torch.nn.utils.clip_grad_norm_([self.tgrad], max_norm)
            self._torch_step(self.tgrad.grad)
        self.pd.copy_(self.p32.detach()[:self.n])
        for k, sd in zip(self.names, self.s):
            sd.copy_(self.state()[k][:self.n])

    def step(self, g, max_norm=0.5, own_clip=False):
        """own_clip: both torch runs step on the gradient torch's clip_grad_norm_ made of g, as the reference does.
        Otherwise they step on the clipped gradient the kernel wrote back (the value its rule saw), which is compared
        with clip_grad_norm_'s right here: torch forms the norm in fp32 and lands a few ulp from the fp64 sum the kernel
        uses, and a coefficient that differs by that much scales the whole gradient, which the fp64 run would hold
        against the kernel at every clipped step.  -> torch's norm"""
        from a2c_amd.optim import nadam_mu_product
        self.step_no += 1
        self.tgrad = g.clone().requires_grad_(True)
        self.tgrad.grad = g.clone()
        tn = float(torch.nn.utils.clip_grad_norm_([self.tgrad], max_norm))
        tstate = {}
        if self.name == "ASGD":      # this step uses the eta / mu the previous one stored (fp32 lr and 1 at first)
            st0 = self.state()
            tstate = dict(eta=float(st0["eta"]), mu=float(st0["mu"])) if st0 else dict(eta=float(np.float32(self.grp["lr"])), mu=1.0)
        if self.name == "NAdam":     # the product after this step: the class's own chain, equal to torch's (asserted below)
            tstate = dict(mu_product=nadam_mu_product(getattr(self, "mu_product", 1.0), self.step_no, self.grp["betas"][0],
                                                      self.grp["momentum_decay"]))
        if own_clip:
            self._torch_step(self.tgrad.grad)
        self.gd.copy_(g)
        self.ops.gradnorm_sq(self.gd, self.sumsq)
        _launch(self.ops, self.name, self.grp, tstate, self.pd, self.gd, self.s, self.sumsq, self.norm, self.step_no,
                max_norm)
        torch.cuda.synchronize()
        tag = f"{self.name} clipped grad step {self.step_no}"
        # against the clip formed in fp64: the norm is one rounding of an fp64 sum (as test_gradnorm_sq_above_its_grid_cap),
        # the gradient four fp32 roundings (norm, + 1e-6, the division, the product) of 6e-8 each, doubled
        n64 = float(g.double().norm())
        assert abs(self.norm.item() - n64) <= 2e-7 * n64 or not np.isfinite(n64)
        close(tag + " (fp64 clip)", self.gd, g.double() * min(1.0, max_norm / (n64 + 1e-6)), 1e-10 * (n64 > 0), 5e-7)
        # against clip_grad_norm_, wherever its own fp32 norm is good to 1e-6 (it is 7e-5 off at 4.2 M elements)
        assert abs(tn - n64) <= 1e-6 * n64 or not np.isfinite(n64) or self.n > 1 << 20, (tn, n64)
        if not abs(tn - n64) > 1e-6 * n64:
            assert self.norm.item() == pytest.approx(tn, rel=2e-6)
            close(tag, self.gd, self.tgrad.grad, 1e-10, 2e-6)
        if not own_clip:
            clipped = self.gd.cpu()
            if self.pool:    # the pool's gradients, times the coefficient the kernel documents (and must reproduce bit for bit)
                c = np.float32(max_norm) / (np.float32(self.norm.item()) + np.float32(1e-6))
                c = torch.tensor(np.float32(1.0) if c > 1 else c)
                assert torch.equal(_bits(clipped), _bits(g * c)), tag
                clipped = torch.cat([clipped, _rand(self.pool, 7000 + self.step_no) * float(g.abs().max()) * c])
            self._torch_step(clipped)
        if self.name == "NAdam":
            assert tstate["mu_product"] == self.mu_product
        return tn

    def check(self, tag, sl=slice(None), states=True):
        """the criterion on the parameters and every state array (elements `sl`), and the sentinels"""
        rows = [("param", self.pd, self.p32, self.p64)]
        if states:
            rows += [(k, sd, self.state()[k], self.state(True)[k]) for k, sd in zip(self.names, self.s)]
        for k, got, t32, t64 in rows:
            if self.pool:
                assert sl == slice(None)
                r = _criterion(f"{self.name} {k} {tag}", got.cpu(), t32.detach(), t64.detach(), self.n)
            else:
                r = _criterion(f"{self.name} {k} {tag}", got.cpu()[sl], t32.detach()[sl], t64.detach()[sl])
            if r is not None:
                self.worst[k] = max(self.worst.get(k, 0.0), r)
        self.sentinels(tag)

    def sentinels(self, tag):
        for k, b in self.buf.items():
            assert bool((b[self.n:].view(torch.int32) == SENTINEL).all()), f"{self.name} {tag}: {k} written past n"

    def report(self, tag):
        print(f"{tag}: worst e_k / e_t " + ", ".join(f"{k} {v:.3f}" for k, v in self.worst.items()))


@pytest.mark.parametrize("name", list(ALL))
def test_clip_kernel_vs_torch_optim(name):
    n = 10007                                        # float4 groups + a 3-element tail
    t, c = _Trio(name, rnd((n,), 220)), _Trio(name, rnd((n,), 220))
    half = torch.arange(n) % 2 == 1
    own = worst = ref = 0
    for step in range(1, STEPS + 1):
        g = rnd((n,), 221 + step) * (0.02 if step == 2 else 0.001)            # step 2 clips, the others do not
        if name == "Rprop":          # odd elements flip sign every step (etaminus, lower clamp), even ones keep it (upper)
            g = rnd((n,), 221).abs() * (0.02 if step == 2 else 0.001) * torch.where(half, torch.tensor(-1.0) ** step, 1.0)
        tn = t.step(g, own_clip=True)                 # torch clips its own gradient, like the reference
        assert t.norm.item() == pytest.approx(tn, rel=2e-6)
        close(f"{name} clipped grad step {step}", t.gd, t.p32.grad, 1e-10, 2e-6)
        close(f"{name} params step {step}", t.pd, t.p32.detach(), 2e-7, 1e-6)
        for k, sd in zip(t.names, t.s):
            want = t.state()[k]
            # (exp_avg's lerp cancels: torch's vectorised CPU path rounds it differently, a few ulp of the array's scale)
            close(f"{name} {k} step {step}", sd, want, 2e-6 * float(want.abs().max()) + 1e-30, 4e-6)
        t.sentinels(f"step {step}")
        own = max(own, _ulps(t.pd, t.p32))
        c.step(g)                                     # the same run with torch stepping on the kernel's clipped gradient
        c.check(f"step {step}")
        worst = max(worst, _ulps(c.pd, c.p32))
        ref = max(ref, _ulps(c.p32, c.p64.float()))
    if name == "Rprop":
        ss = t.state()["step_size"]
        assert float(ss.min()) == pytest.approx(5e-4) and float(ss.max()) == pytest.approx(1.3e-3)   # both clamps
    if name == "ASGD":
        assert float(t.state()["mu"]) != 1.0
    if name == "RAdam":
        assert 1 < _radam_first_rectified(t.grp["betas"]) <= STEPS
    # `own` is not bounded: from step 2 on it holds the few ulp by which clip_grad_norm_'s fp32 norm misses the fp64 one
    print(f"{name}: max param difference {worst} ulp over {STEPS} steps (torch fp32 from fp64 rounded to fp32: {ref} ulp; "
          f"against torch stepping on its own clip: {own} ulp)")
    c.report(f"{name} hashed p0 of size 1")
    assert worst <= 2 * ref + 1


# ------------------------------------------------------------------ the criterion at three parameter scales, 12 steps
SCALES = {"1": 1.0, "1e-3": 1e-3, "0": 0.0}       # at 0 the parameter IS the accumulated update
VARIANTS = {**{n: (n, None) for n in ALL},
            "Adagrad-lr_decay": ("Adagrad", dict(lr_decay=0.3)),          # clr = lr / 1.3 at step 2
            "ASGD-t0_default": ("ASGD", {})}                             # t0 = 1e6: mu stays 1, ax copies the parameters


@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_precision_against_fp64(variant, scale):
    name, group = VARIANTS[variant]
    n = 10007
    t = _Trio(name, _rand(n, 300) * SCALES[scale], group)
    mus = set()
    for k in range(1, STEPS + 1):
        t.step(_grad(name, n, k, 310))
        t.check(f"step {k}")
        if name == "ASGD":
            mus.add(float(t.state()["mu"]))
    if variant == "Adagrad-lr_decay":
        assert t.grp["lr_decay"] == 0.3
    if variant == "ASGD-t0_default":
        assert t.grp["t0"] == 1e6 and mus == {1.0} and torch.equal(t.s[0].cpu(), t.pd.cpu())
    if variant == "ASGD":
        assert len(mus) >= 8                          # 1, 1/2, ..., 1/10: the averaging weight changes every step past t0
    t.report(f"{variant} p0 of size {scale}")


@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("betas", [None, (0.9, 0.99), (0.9, 0.8)], ids=["default", "beta2_0.99", "beta2_0.8"])
def test_radam_crosses_the_rectification_threshold(betas, scale):
    n = 10007
    t = _Trio("RAdam", _rand(n, 320) * SCALES[scale], {} if betas is None else dict(betas=betas))
    first = _radam_first_rectified(t.grp["betas"])
    assert 1 < first < STEPS                          # rho_t crosses 5 inside the run
    for k in range(1, STEPS + 1):
        t.step(_grad("RAdam", n, k, 330))
        t.check({first - 1: "last unrectified ", first: "first rectified "}.get(k, "") + f"step {k}")
    print(f"RAdam betas {t.grp['betas']}: first rectified step {first}")
    t.report(f"RAdam betas {t.grp['betas']} p0 of size {scale}")


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024])   # tail only, one float4 group, group + tail, no tail
@pytest.mark.parametrize("name", list(ALL))
def test_clip_kernel_small_sizes(name, n):
    t = _Trio(name, _rand(n, 400) * 1e-3, pool=4096 if n < 1023 else 0)
    for k in range(1, STEPS + 1):
        t.step(_grad(name, n, k, 410))
        t.check(f"n {n} step {k}")


# a2c_grid_1d caps the step kernels at 2048 workgroups x 256 threads x one float4 = 2 097 152 elements per pass
BIG_N = 2 * 2097152 + 4099                                  # two full grid-stride passes, a partial third, a 3-element tail


@pytest.mark.parametrize("name", list(ALL))
def test_clip_kernel_three_grid_stride_passes(name):
    n = BIG_N
    t = _Trio(name, _rand(n, 500) * 1e-3)
    if name == "RAdam":                                       # starts at step 5 so that the 3 steps cross rho_t = 5
        t.warm([_grad(name, n, k, 505) for k in range(1, 6)])
        assert t.step_no < _radam_first_rectified(t.grp["betas"]) <= t.step_no + 3
    for k in range(1, 4):
        t.step(_grad(name, n, k, 510))
        t.check(f"n {n} step {k}")
    t.report(f"{name} n {n}")


def test_gradnorm_sq_above_its_grid_cap():
    from a2c_amd import ops
    n = 3 * 1048576 + 7             # its cap is 1024 workgroups x 256 threads x one float4 = 1 048 576 elements per pass
    g = _rand(n, 600)
    want = float(np.sqrt(np.sum(g.numpy().astype(np.float64) ** 2)))
    gbuf, pbuf = _dev(n), _dev(n)
    gbuf[:n].copy_(g)
    scratch = ops.new_reduce_scratch(gbuf.device)
    out = torch.zeros(3, dtype=torch.float64, device=DEV)
    ops.gradnorm_sq(gbuf[:n], out[0:1], scratch=scratch)
    ops.gradnorm_sq(gbuf[:n], out[1:2], scratch=scratch)      # the first call's last workgroup reset the ticket counter
    ops.gradnorm_sq(gbuf[:n // 2], out[2:3], scratch=scratch)
    norm = torch.zeros(1, device=DEV)
    ops.clip_sgd(pbuf[:n], gbuf[:n], out[0:1], 1e30, 1e-3, norm)
    torch.cuda.synchronize()
    first, second, part = (float(v) for v in np.sqrt(out.cpu().numpy()))
    want_part = float(np.sqrt(np.sum(g.numpy()[:n // 2].astype(np.float64) ** 2)))
    print(f"gradnorm n {n}: {first!r} {second!r} fp64 {want!r} rel {abs(first - want) / want:.2e}")
    # the sum is formed in fp64 and only the final cast rounds: one fp32 ulp (6e-8 relative), doubled
    assert first == second and abs(first - want) <= 2e-7 * want
    assert abs(part - want_part) <= 2e-7 * want_part
    assert abs(norm.item() - want) <= 2e-7 * want
    assert torch.equal(_bits(gbuf[:n]), _bits(g))           # coefficient 1: written back bit-identical
    for b in (gbuf, pbuf):
        assert bool((b[n:].view(torch.int32) == SENTINEL).all())


# ------------------------------------------------------------------ values
def _value_classes(layout):
    """element classes in blocks of 13 (three float4 groups + 1, so the blocks start at every offset within a group):
    115 elements that end in three whose classes depend on the layout, 65 times over (each class has enough elements for
    its own e_t to mean something): n = 7475 = 4 * 1868 + 3, so those three are the kernel's scalar tail"""
    cls = np.concatenate([np.full(13, c) for c in range(5)] + [np.full(41, 5), np.full(6, 6)])
    return np.tile(np.concatenate([cls, np.array(((0, 2, 5), (1, 3, 4))[layout])]), 65)


def _value_grad(cls, k, seed):
    """step k = 1..4 of each class:
    0: +0, +0, x, +0        Rprop: prev == 0 and g == 0; g != 0 on prev == 0; sign(0) on a non-zero prev
    1: -0, x, -x, +0        Rprop: s == 0, then s < 0 (prev is zeroed), then g == 0 on that zeroed prev
    2: +1e-30               g * g and g * prev underflow to 0
    3: -/+ 1e-30            ... with the sign alternating
    4: +-3e-20              g * g is a denormal
    5: generic              6: +-(5 .. 10)"""
    n = len(cls)
    x, x1 = 0.1 * _rand(n, seed + k).numpy(), 0.1 * _rand(n, seed).numpy()
    sgn = np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.float32)
    vals = [(0.0, 0.0, x, 0.0)[k - 1], (-0.0, x1, -x1, 0.0)[k - 1], 1e-30, -1e-30 * (-1.0) ** k, 3e-20 * sgn, x, (5 + 50 * np.abs(x1)) * sgn]
    g = np.zeros(n, np.float32)
    for c, v in enumerate(vals):
        g[cls == c] = np.broadcast_to(np.float32(v), n)[cls == c]
    return torch.from_numpy(g)


@pytest.mark.parametrize("name", list(ALL))
def test_zeros_underflow_and_large_values(name):
    for layout in (0, 1):
        cls = _value_classes(layout)
        n = len(cls)
        assert n % 4 == 3
        # max_norm 1e4: the coefficient is exactly 1 and the kernel sees the values above; 0.5: they are scaled by ~3e-3
        for max_norm in (1e4, 0.5):
            t = _Trio(name, _rand(n, 800 + layout))
            for k in range(1, 5):
                g = _value_grad(cls, k, 810)
                if k == 1:
                    assert bool(np.signbit(g.numpy()[cls == 1]).all()) and not np.signbit(g.numpy()[cls == 0]).any()
                old32, oldk = _bits(t.p32), _bits(t.pd)
                t.step(g, max_norm)
                tag = f"layout {layout} max_norm {max_norm} step {k}"
                t.check(tag)
                # ... and the parameters of each class on their own, so that the +-10 do not set the scale for the 1e-30.
                # (Not the state arrays: exp_avg of class 3 cancels to a few 1e-32, where the functor's product-then-sum
                # and torch's lerp_, one fused multiply-add, differ by 8.18 e_t, measured: 3e-9 of the gradient.)
                for c in range(7):
                    t.check(f"{tag} class {c}", torch.from_numpy(cls == c), states=False)
                # where torch's fp32 parameter is exactly unchanged, so is the kernel's
                same = _bits(t.p32) == old32
                assert torch.equal(_bits(t.pd)[same], oldk[same]), tag
                if name in ("SGD", "Rprop", "Adagrad"):          # a zero gradient does not move a parameter
                    zero = g == 0
                    assert bool(same[zero].all()) and torch.equal(_bits(t.pd)[zero], oldk[zero]), tag
            assert not torch.equal(_bits(t.pd), _bits(_rand(n, 800 + layout)))     # it did step
    t.report(f"{name} signed zeros, underflow, +-10")


CLIP_CASES = {"zero": 0.0, "below": 0.5 * (1 - 2.0 ** -20), "above": 0.5 * (1 + 2.0 ** -20),
              # ... and on each side of the norm at which max_norm / (norm + 1e-6) is 1
              "clamp_below": (0.5 - 1e-6) * (1 - 2.0 ** -20), "clamp_above": (0.5 - 1e-6) * (1 + 2.0 ** -20), "huge": 1e6}


@pytest.mark.parametrize("case", list(CLIP_CASES))
@pytest.mark.parametrize("name", list(ALL))
def test_clip_coefficient_edges(name, case):
    n = 10007
    g = torch.zeros(n) if case == "zero" else _with_norm(_rand(n, 700), CLIP_CASES[case])
    t = _Trio(name, _rand(n, 701))
    tn = t.step(g)
    if case == "zero":
        assert t.norm.item() == 0.0 and tn == 0.0
        assert torch.equal(_bits(t.gd), torch.zeros(n, dtype=torch.int32))     # written back as (+)zeros
    t.check(case)


@pytest.mark.parametrize("name", ["SGD", "Adam", "RMSprop"])
def test_one_inf_gradient_poisons_what_torch_poisons(name):
    """norm inf, coefficient 0: inf * 0 = NaN at that element, (signed) zeros elsewhere"""
    n = 10007
    g = _grad(name, n, 1, 720)
    g[4321] = float("inf")
    t = _Trio(name, _rand(n, 721))
    t.step(_grad(name, n, 1, 719))
    t.step(g)
    assert np.isinf(t.norm.item())
    rows = [("grad", t.gd, t.p32.grad), ("param", t.pd, t.p32)] + [(k, sd, t.state()[k]) for k, sd in zip(t.names, t.s)]
    for k, got, want in rows:
        got, want = got.detach().cpu(), want.detach()
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(got), fin) and torch.equal(torch.isnan(got), torch.isnan(want)), (name, k)
        close(f"{name} {k} finite part", got[fin], want[fin], 2e-7, 4e-6)
    assert int((~torch.isfinite(t.p32.detach())).sum()) == 1


def _fc_updater(name, group=None):
    from a2c_amd.updater import Updater
    kind, ss, A, h, R_, T, _ = FC
    upd = Updater(make_net(kind, ss, A, h), base_hyps(n_tsteps=T, n_rollouts=R_, optim_type=name, h_size=h))
    upd.optim.param_groups[0].update(group or {})
    return upd


@pytest.mark.parametrize("name", list(ALL))
def test_max_norm_none_leaves_the_gradient_bit_identical(name):
    upd = _fc_updater(name)
    ar = upd.net._arena
    for g in (_with_norm(_rand(ar.n_train, 730), 1e6), _value_grad(np.arange(ar.n_train) % 7, 2, 731)):
        ar.train_grads().copy_(g)
        before = ar.train_params().clone()
        upd.optim.step(max_norm=None)
        torch.cuda.synchronize()
        assert torch.equal(_bits(ar.train_grads()), _bits(g))
        assert float(upd.optim.grad_norm()) == pytest.approx(float(g.double().norm()), rel=2e-7)
        assert not torch.equal(ar.train_params(), before)


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


# ------------------------------------------------------------------ the host classes' step-dependent scalars over many updates
# the rules whose launch arguments depend on the step count, or on fp32 scalars the class carries from step to step
HOSTED = {"Adam": ("Adam", {}), "AdamW": ("AdamW", {}), "Adamax": ("Adamax", {}), "NAdam": ("NAdam", {}),
          "RAdam": ("RAdam", {}), "ASGD": ("ASGD", {}), "ASGD-t0_4": ("ASGD", dict(t0=4.0)),
          "Adagrad-lr_decay": ("Adagrad", dict(lr_decay=0.3))}
CHECK_AT = (1, 5, 6, 7, 20, 40)


def _host_grad(ar, k):
    """a flat gradient over the trainable prefix, zero in its alignment padding (no parameter's state lives there);
    clipped at updates 2, 9 and 25"""
    g = torch.zeros(ar.n_train)
    for name in ar.trainable:
        o, cnt, _ = ar.offsets[name]
        g[o:o + cnt] = _rand(cnt, 900 + 50 * k + o % 47)
    return _with_norm(g, 2.0 if k in (2, 9, 25) else 0.05)


def _host_scalars(optim):
    """{(scalar, value)} over the trainable parameters of a published state: one value each"""
    optim.state_dict()
    sts = [optim.state[p] for p in optim.param_groups[0]["params"] if optim._trainable(p)]
    return {k: {float(st[k]) for st in sts} for k in ("step",) + tuple(optim._scalars)}


@pytest.mark.parametrize("variant", list(HOSTED))
def test_host_class_40_updates_vs_torch(variant):
    name, group = HOSTED[variant]
    upd = _fc_updater(name, group)
    ar = upd.net._arena
    n = ar.n_train
    p0 = ar.train_params().detach().cpu().clone()            # the flat trainable prefix (alignment padding included)
    p32, p64 = p0.clone().requires_grad_(True), p0.double().requires_grad_(True)
    lr = upd.optim.param_groups[0]["lr"]
    opt32, opt64 = (getattr(torch.optim, name)([p], lr=lr) for p in (p32, p64))
    for o in (opt32, opt64):
        o.param_groups[0].update(group)
    worst = 0.0
    for k in range(1, 41):
        g = _host_grad(ar, k)
        p32.grad = g.clone()
        tn = float(torch.nn.utils.clip_grad_norm_([p32], 0.5))
        opt32.step()
        p64.grad = p32.grad.double()
        opt64.step()
        ar.train_grads().copy_(g)
        upd.optim.step(max_norm=0.5)
        if k in CHECK_AT:
            torch.cuda.synchronize()
            assert float(upd.optim.grad_norm()) == pytest.approx(tn, rel=2e-6)
            r = _criterion(f"{variant} update {k}", ar.train_params(), p32, p64)
            worst = max(worst, r or 0.0)
            got, want = _host_scalars(upd.optim), opt32.state[p32]
            assert got == {s: {float(want[s])} for s in got}, (variant, k, got)
    print(f"{variant}: worst e_k / e_t of the parameters over updates {CHECK_AT}: {worst:.3f}")


STRADDLE = {"RAdam": ("RAdam", {}), "NAdam": ("NAdam", {}), "ASGD-t0_4": ("ASGD", dict(t0=4.0))}


@pytest.mark.parametrize("variant", list(STRADDLE))
def test_checkpoint_straddles_a_branch(variant):
    """state_dict() after update 5 into a fresh Updater: updates 6..8 equal the uninterrupted run's bit for bit.  Update 6
    is RAdam's first rectified one; with t0 = 4 update 5 is the last to store ASGD's mu = 1 and 7 the first to average."""
    name, group = STRADDLE[variant]
    if name == "RAdam":
        assert _radam_first_rectified(_fc_updater(name).optim.param_groups[0]["betas"]) == 6

    def run(upd, ks):
        out = []
        for k in ks:
            upd.net._arena.train_grads().copy_(_host_grad(upd.net._arena, k))
            upd.optim.step(max_norm=0.5)
            torch.cuda.synchronize()
            out.append((upd.net._arena.params.clone(), {s: v.clone() for s, v in upd.optim._flat.items()},
                        dict(upd.optim._scal), _host_scalars(upd.optim)))
        return out

    a = _fc_updater(name, group)
    run(a, range(1, 6))
    sd, params = copy.deepcopy(a.optim.state_dict()), a.net._arena.params.clone()
    want = run(a, range(6, 9))
    b = _fc_updater(name)                                     # the loaded param_group carries t0
    b.net._arena.params.copy_(params)
    b.net.mark_dirty()
    b.optim.load_state_dict(sd)
    assert b.optim._steps == 5
    assert all(b.optim.param_groups[0][k] == v for k, v in a.optim.param_groups[0].items() if k != "params")
    got = run(b, range(6, 9))
    if name == "ASGD":
        assert [w[2]["mu"] for w in want] == [0.5, float(np.float32(1 / 3)), 0.25]
    if name == "NAdam":
        assert len({w[2]["mu_product"] for w in want}) == 3
    for k, ((pa, fa, sa, ha), (pb, fb, sb, hb)) in enumerate(zip(want, got), 6):
        assert torch.equal(pa, pb), (variant, k)
        assert fa.keys() == fb.keys() and all(torch.equal(fa[s], fb[s]) for s in fa), (variant, k)
        assert sa == sb and ha == hb, (variant, k)


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
