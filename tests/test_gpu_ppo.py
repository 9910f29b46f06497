"""The clipped multi-epoch update (hyps["ppo_epochs"] / hyps["ppo_clip"]) on the MI355X.

Kernels: a2c_ppo_loss_fwd_bwd and a2c_gauss_ppo_fwd_bwd against a torch statement of the loss written here (log-softmax /
torch.distributions.Normal, minimum, clamp, autograd) in float64, with its float32 run as the twin, under the criterion of
tests/test_gpu_small_kernels.py (e_k <= 2 e_t + ulp(scale)); record mode against the sibling kernels bit for bit; use mode
at r == 1 against record mode bit for bit; determinism, an overflowing ratio, shares, argument checks.

The update: K = 3 epochs against a float64 restatement (net, scan, clipped loss with logp_old detached from epoch 0,
clip_grad_norm_, torch.optim); ppo_epochs = 1 is today's update; the dispatcher path; captured == eager; the refusals; and
the one-state bandit of tests/test_gpu_gauss_exact.py with four epochs a rollout."""
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
from cases import O, base_hyps, hashf
from test_gpu_gauss_exact import (BANDIT_ROWS, BANDIT_TARGET, BANDIT_UPDATES, RAW_BIAS, UPDATE_H, UPDATE_R, UPDATE_T,
                                  bandit_hyps, info_bound_ratio, net64, param_bound_ratio, rand_heads, scan64)

pytestmark = pytest.mark.gpu
DEV = "cuda"
PC, VC, EC = 0.8, 0.5, 0.01
CLIP = 0.2
POOL = 512                         # rows of the two torch runs where the kernel sees fewer (test_gpu_small_kernels.py)
SENT = 12345.6787109375            # sentinel value (an exact float32) of every padded output
PPO_BLOCK_CAP = 512                # the two launches' grid cap (include/a2c_mi355x.h): above 256 x this, a second trip
GAP = 120.0                        # expf(-120) = 0 in fp32
# logp_old = logp64 - d: the log-ratios.  clip = 0.2 has its edges at log 0.8 = -0.223 and log 1.2 = +0.182
D_CYCLE = torch.tensor([0.0, 0.05, -0.05, 0.15, -0.15, 0.5, -0.5, 2.0, -2.0], dtype=torch.float64)
EDGE_MARGIN = 0.03
_RATIOS = {}


# ------------------------------------------------------------------------------------------------- the criterion
def _crit(tag, got, t32, t64, scale=None):
    """e_k <= 2 e_t + ulp(scale) (tests/test_gpu_small_kernels.py::_crit): e_t the fp32 twin's deviation from fp64, scale the
    magnitude of the largest term summed into an element (default max |fp64|) -> e_k / e_t.  As there, `got` may be the
    leading rows of what the two torch runs cover (POOL rows where the kernel sees fewer)."""
    t64 = t64.detach().double().reshape(-1)
    t32 = t32.detach().double().reshape(-1)
    g = got.detach().cpu().double().reshape(-1)
    n = g.numel()
    assert n <= t64.numel() and t32.numel() == t64.numel(), (tag, n, t32.numel(), t64.numel())
    e_k = float((g - t64[:n]).abs().max())
    e_t = float((t32 - t64).abs().max())
    scale = float(t64.abs().max()) if scale is None else float(scale)
    ulp = float(np.spacing(np.float32(scale)))
    ratio = e_k / e_t if e_t > 0 else None
    print(f"    {tag}: e_k {e_k:.3e} e_t {e_t:.3e} ulp {ulp:.3e} e_k/e_t {ratio if ratio is None else round(ratio, 3)}")
    assert e_k <= 2 * e_t + ulp, f"{tag}: e_k {e_k:.3e} > 2 * e_t {e_t:.3e} + ulp {ulp:.3e}"
    if ratio is not None:
        k = tag.split(":")[0].split(" ")[0]
        _RATIOS[k] = max(_RATIOS.get(k, 0.0), ratio)
    return ratio


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    yield
    print("\nworst e_k / e_t per array over this run:")
    for k in sorted(_RATIOS):
        print(f"  RATIO {k} {_RATIOS[k]:.3f}")


SUM_TERMS = ("t_pi", "t_val", "t_ent", "t_clip", "t_kl")


def _check_sums(tag, s, r32, r64, rows=slice(None), which=range(5)):
    """the fp64 sums against the fp64 sum of the per-row terms (tests/test_gpu_small_kernels.py::_check_loss_sums): every
    row's term is allowed 2 e_t + ulp (e_t of the fp32 per-row terms, ulp at the largest term), the sum n times that"""
    for i in which:
        k = SUM_TERMS[i]
        t64 = r64[k][rows].double()
        n = t64.numel()
        e_t = float((r32[k].double() - r64[k]).abs().max())
        ulp = float(np.spacing(np.float32(r64[k].abs().max())))
        want = float(t64.sum())
        e_k = abs(float(s[i]) - want)
        print(f"    {tag} sum {k}: |kernel - fp64| {e_k:.3e}, bound {n * (2 * e_t + ulp):.3e}")
        assert e_k <= n * (2 * e_t + ulp), (tag, k, float(s[i]), want)


# ------------------------------------------------------------------------------------------------- the yardstick
def ppo_terms(logp, logp_old, w, clip):
    """the clipped surrogate in the dtype of its arguments -> (r, surr, keep)"""
    r = (logp - logp_old).exp()
    surr = torch.minimum(r * w, torch.clamp(r, 1 - clip, 1 + clip) * w)
    keep = ~(((w > 0) & (r > 1 + clip)) | ((w < 0) & (r < 1 - clip)))
    return r, surr, keep


def policy_rows(kind, x, acts, n):
    """-> (logp of the taken action, minus the entropy) per row.  kind 'd': x logits, acts int64 (-1 = the last action);
    kind 'g': x rows [mu (n) | raw (n)], acts (N, n), a diagonal Gaussian with sigma = softplus(raw) + 1e-4"""
    if kind == "d":
        lsm = F.log_softmax(x, dim=-1)
        return lsm[torch.arange(len(acts)), acts], (lsm * F.softmax(x, dim=-1)).sum(-1)
    dist = torch.distributions.Normal(x[:, :n], F.softplus(x[:, n:2 * n]) + 1e-4)
    return dist.log_prob(acts.to(x.dtype)).sum(-1), -dist.entropy().sum(-1)


def ppo_ref(kind, x, v, acts, advs, rets, logp_old, n, norm, clip, dtype, N, pi_coef=PC):
    """the loss in `dtype` over the first N rows as the batch (means are sums / N); rows past N are the pool: same
    statistics, same 1 / N (test_gpu_small_kernels.py::_loss_ref).  logp_old None = record mode (r = 1: the ratio of logp to
    its own detached value) -> per-row terms and gradients"""
    x = x.to(dtype).clone().requires_grad_(True)
    v = v.to(dtype).clone().requires_grad_(True)
    w = advs.to(dtype)
    if norm:
        w = (w - w[:N].mean()) / (w[:N].std() + 1e-6)
    logp, t_ent = policy_rows(kind, x, acts, n)
    old = logp.detach() if logp_old is None else logp_old.to(dtype)
    r, surr, keep = ppo_terms(logp, old, w, clip)
    t_val = (v - rets.to(dtype)) ** 2
    loss = pi_coef * -(surr.sum() / N) + VC * (t_val.sum() / N) + EC * (t_ent.sum() / N)
    loss.backward()
    rd = r.detach()
    return dict(t_pi=surr.detach(), t_val=t_val.detach(), t_ent=t_ent.detach(), t_clip=(~keep).to(dtype),
                t_kl=(rd - 1) - (logp.detach() - old), dx=x.grad, dv=v.grad, w=w.detach(), r=rd, keep=keep, logp=logp.detach())


def grad_scale(kind, x, acts, r64, n, N, pi_coef=PC):
    """the largest term summed into an element of the policy gradient array, from the fp64 run"""
    x = x.double()
    gpi = pi_coef * (r64["w"] * r64["r"] * r64["keep"]).abs() / N
    if kind == "d":
        lsm = F.log_softmax(x, dim=-1)
        p = lsm.exp()
        A = x.shape[1]
        onehot = F.one_hot(torch.where(acts < 0, acts + A, acts), A).double()
        ta = gpi[:, None] * (onehot - p).abs()
        tb = EC / N * (p * (lsm - r64["t_ent"][:, None])).abs()
        return max(float(ta.max()), float(tb.max()))
    # dmu = gpi u / sigma (one product); draw = (gpi u^2 - gpi - entr_coef / N) / sigma * softplus'(raw): three terms
    raw = x[:, n:2 * n]
    sg = F.softplus(raw) + 1e-4
    u = ((acts.double() - x[:, :n]) / sg).abs()
    g = gpi[:, None]
    t_mu = g * u / sg
    t_raw = torch.maximum(g * torch.clamp(u * u, min=1.0), torch.full_like(u, EC / N)) / sg * torch.sigmoid(raw)
    return max(float(t_mu.max()), float(t_raw.max()))


# ------------------------------------------------------------------------------------------------- inputs
def discrete_inputs(N, A, seed):
    """logits in the regimes of test_gpu_small_kernels.py::_loss_inputs: every tenth row or so has one logit GAP above the
    rest (half of them act on it, half on another), another tenth has all logits equal, a seventh of the actions are -1"""
    g = torch.Generator().manual_seed(seed)
    lg = (torch.rand(N, A, generator=g, dtype=torch.float64) * 6 - 3).float()
    kind = torch.randint(0, 10, (N,), generator=g)
    acts = torch.randint(0, A, (N,), generator=g)
    dom = torch.randint(0, A, (N,), generator=g)
    rows = (kind == 0).nonzero().flatten()
    lg[rows, dom[rows]] += GAP
    acts[rows[::2]] = dom[rows[::2]]
    lg[kind == 1] = 0.5
    acts[torch.randint(0, 7, (N,), generator=g) == 0] = -1
    v = torch.randn(N, generator=g)
    advs = torch.randn(N, generator=g) * 1.5 + 0.3
    rets = torch.randn(N, generator=g)
    return lg, v, acts, advs, rets


def gauss_inputs(N, n, seed):
    """heads as rand_heads of test_gpu_gauss_exact.py (every regime of the softplus and of sigma), on-policy actions"""
    heads = rand_heads(N, n, seed)
    g = torch.Generator().manual_seed(seed * 7 + n)
    acts = heads[:, :n] + (F.softplus(heads[:, n:2 * n]) + 1e-4) * torch.randn(N, n, generator=g)
    advs, rets = torch.randn(N, generator=g), torch.randn(N, generator=g)
    return heads[:, :2 * n].contiguous(), heads[:, 2 * n].contiguous(), acts, advs, rets


def make_case(kind, N, n, norm, seed):
    """max(N, POOL) rows of inputs (the kernel sees the first N), logp_old = logp64 - d with d cycling through D_CYCLE, and
    the four torch runs (record / use x fp64 / fp32); asserts the two conditions on the inputs: the twin's keep is the fp64
    keep on every row, and (N >= 255) all five situations occur"""
    Np = max(N, POOL)
    x, v, acts, advs, rets = (discrete_inputs if kind == "d" else gauss_inputs)(Np, n, seed)
    rec64 = ppo_ref(kind, x, v, acts, advs, rets, None, n, norm, CLIP, torch.float64, N)
    rec32 = ppo_ref(kind, x, v, acts, advs, rets, None, n, norm, CLIP, torch.float32, N)
    d = D_CYCLE[(torch.arange(Np) + 1) % len(D_CYCLE)]          # (row 0: 0.05, so that a batch of one row has r != 1)
    logp_old = rec64["logp"] - d
    use64 = ppo_ref(kind, x, v, acts, advs, rets, logp_old, n, norm, CLIP, torch.float64, N)
    use32 = ppo_ref(kind, x, v, acts, advs, rets, logp_old, n, norm, CLIP, torch.float32, N)
    lr = use64["r"].log()
    assert float(torch.minimum((lr - np.log1p(CLIP)).abs(), (lr - np.log1p(-CLIP)).abs()).min()) >= EDGE_MARGIN
    assert torch.equal(use32["keep"], use64["keep"]), "the fp32 twin clips another set of rows than fp64"
    if N >= 255:
        w, r, keep = use64["w"][:N], use64["r"][:N], use64["keep"][:N]
        hi, lo = r > 1 + CLIP, r < 1 - CLIP
        for sel, kept in ((~hi & ~lo, True), ((w > 0) & hi, False), ((w < 0) & lo, False), ((w > 0) & lo, True),
                          ((w < 0) & hi, True)):
            assert sel.any() and bool((keep[sel] == kept).all())
    # x .. logp_old: the N rows the kernel sees; px, pacts and the four torch runs: the pool
    return dict(kind=kind, N=N, n=n, norm=norm, x=x[:N], v=v[:N], acts=acts[:N], advs=advs[:N], rets=rets[:N],
                logp_old=logp_old[:N], px=x, pacts=acts, rec64=rec64, rec32=rec32, use64=use64, use32=use32)


class Dev:
    """the device side of a case, every 2-D argument strided: heads rows [x | value | guard] (the value column's stride is
    the row's), Gaussian actions in a wider buffer, the gradient buffer full of sentinels with a guard column behind dV and
    two guard rows"""

    def __init__(self, c):
        self.c = c
        kind, N, W = c["kind"], c["N"], c["x"].shape[1]
        self.W = W
        self.hb = torch.full((N, W + 2), SENT, device=DEV)
        self.hb[:, :W] = c["x"].to(DEV)
        self.hb[:, W] = c["v"].to(DEV)
        if kind == "d":
            self.acts = c["acts"].to(DEV)
        else:
            self.acts = torch.full((N, c["n"] + 1), SENT, device=DEV)
            self.acts[:, :c["n"]] = c["acts"].to(DEV)
        self.advs, self.rets = c["advs"].to(DEV), c["rets"].to(DEV)
        self.asum = None
        if c["norm"]:
            self.asum = torch.zeros(2, dtype=torch.float64, device=DEV)
            ops.moments(self.advs, self.asum)

    def run(self, record, logp_old=None, lo=0, hi=None, pi_coef=PC, sibling=False, clip=CLIP):
        """one launch on rows lo:hi with n_global = N -> (sums on the host, the whole gradient buffer, logp_old)"""
        c, W, N = self.c, self.W, self.c["N"]
        hi = N if hi is None else hi
        db = torch.full((N + 2, W + 2), SENT, device=DEV)
        lp = torch.full((N + 2,), SENT, dtype=torch.float64, device=DEV) if logp_old is None else logp_old
        s = torch.full((3 if sibling else 5,), float("nan"), dtype=torch.float64, device=DEV)
        rows = slice(lo, hi)
        a = self.acts[rows] if c["kind"] == "d" else self.acts[rows, :c["n"]]
        head = (self.hb[rows, :W], self.hb[rows, W], a, self.advs[rows], self.rets[rows], self.asum, N)
        if c["kind"] == "g":
            head += (c["n"],)
        out = (db[rows, :W], db[rows, W], s)
        if sibling:
            (ops.loss_fwd_bwd if c["kind"] == "d" else ops.gauss_nll_fwd_bwd)(*head, pi_coef, VC, EC, *out)
        else:
            (ops.ppo_loss_fwd_bwd if c["kind"] == "d" else ops.gauss_ppo_fwd_bwd)(*head, pi_coef, VC, EC, clip, record, lp[rows],
                                                                                 *out)
        torch.cuda.synchronize()
        return s.cpu(), db, lp

    def guards_intact(self, db, lp=None, lo=0, hi=None):
        N, W = self.c["N"], self.W
        hi = N if hi is None else hi
        ok = bool((db[:, W + 1] == SENT).all()) and bool((db[:lo] == SENT).all()) and bool((db[hi:] == SENT).all())
        if lp is not None:
            ok = ok and bool((lp[:lo] == SENT).all()) and bool((lp[hi:] == SENT).all())
        return ok


_CASES = {}


def case(kind, N, n, norm):
    """the reference of a case is computed once and shared by the tests that need it (they never write it)"""
    key = (kind, N, n, norm)
    if key not in _CASES:
        _CASES[key] = make_case(kind, N, n, norm, 4000 + 31 * n + N % 977 + int(norm))
    return _CASES[key]


BIG_N = 256 * PPO_BLOCK_CAP + 77           # the grid-stride loop's second trip
KERNEL_CASES = ([("d", N, A, norm) for A in (1, 2, 6, 32) for N in (1, 255, 257, 1000) for norm in (False, True) if N > 1 or not norm]
                + [("g", N, n, norm) for n in (1, 3, 64) for N in (1, 255, 257, 1000) for norm in (False, True) if N > 1 or not norm]
                + [("d", BIG_N, 6, True), ("g", BIG_N, 3, True)])


# ------------------------------------------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("kind,N,n,norm", KERNEL_CASES)
def test_kernels_record_and_use_modes(kind, N, n, norm):
    """properties 1-4: record mode is the sibling kernel bit for bit and writes logp_old; use mode on what record mode wrote
    is record mode bit for bit (r == 1); use mode against the fp64 yardstick; two identical calls agree bit for bit"""
    c = case(kind, N, n, norm)
    dv = Dev(c)
    W = dv.W
    tag = f"{'ppo' if kind == 'd' else 'gauss_ppo'}"
    # 1. record mode
    s_sib, d_sib, _ = dv.run(True, sibling=True)
    s_rec, d_rec, lp_rec = dv.run(True)
    assert dv.guards_intact(d_rec, lp_rec) and dv.guards_intact(d_sib)
    assert torch.equal(d_rec, d_sib), "record mode's gradients differ from the sibling kernel's"
    assert torch.equal(s_rec[1:3], s_sib[1:3])
    assert float(s_rec[3]) == 0.0 and float(s_rec[4]) == 0.0
    term = None
    if kind == "g":     # the largest term summed into a row's logp: u^2 / 2, log sigma or log(2 pi) / 2 of one dim
        sg = F.softplus(c["px"][:, n:].double()) + 1e-4
        term = float(torch.maximum(0.5 * ((c["pacts"].double() - c["px"][:, :n].double()) / sg) ** 2, sg.log().abs()).max())
        term = max(term, 0.919)
    _crit(f"{tag}.logp_old", lp_rec[:N], c["rec32"]["logp"], c["rec64"]["logp"], term)
    rec_w = dict(t_pi=c["rec64"]["w"]), dict(t_pi=c["rec32"]["w"])
    _check_sums(f"{tag} record", s_rec, rec_w[1], rec_w[0], slice(0, N), which=[0])           # sums[0] = sum w_i
    # 2. use mode at r == 1
    s_one, d_one, _ = dv.run(False, logp_old=lp_rec)
    assert torch.equal(d_one, d_rec) and torch.equal(s_one, s_rec), "use mode at r == 1 differs from record mode"
    # 3. use mode against the yardstick; 4. twice
    lp = torch.full((N + 2,), SENT, dtype=torch.float64, device=DEV)
    lp[:N] = c["logp_old"].to(DEV)
    (s0, d0, _), (s1, d1, _) = (dv.run(False, logp_old=lp) for _ in range(2))
    assert torch.equal(s0, s1) and torch.equal(d0, d1), "two identical calls differ"
    assert dv.guards_intact(d0) and torch.equal(lp[:N].cpu(), c["logp_old"]) and bool((lp[N:] == SENT).all())
    r64, r32 = c["use64"], c["use32"]
    _crit(f"{tag}.dpolicy", d0[:N, :W], r32["dx"], r64["dx"], grad_scale(kind, c["px"], c["pacts"], r64, n, N))
    _crit(f"{tag}.dvals", d0[:N, W], r32["dv"], r64["dv"])
    _check_sums(f"{tag} use", s0, r32, r64, slice(0, N))
    assert float(s0[3]) == float(r64["t_clip"][:N].sum())


@pytest.mark.parametrize("kind,n", [("d", 6), ("g", 3), ("g", 64)])
def test_overflowing_ratio_on_a_clipped_row(kind, n):
    """rows with logp - logp_old = +200 (r = 7e86: inf as a float) and +800 (inf in fp64 too) and w > 0: the clip binds, so
    the policy part of the row's gradient is a selected zero -- the row equals its gradient at pi_coef = 0 and is finite"""
    N = 257
    c = dict(case(kind, N, n, False))
    rows = [3, 130, 256]
    c["advs"] = c["advs"].clone()
    c["advs"][rows] = torch.tensor([1.5, 0.25, 3.0])
    dv = Dev(c)
    lp = c["logp_old"].clone()
    lp[rows] = c["rec64"]["logp"][rows] - torch.tensor([200.0, 800.0, 200.0], dtype=torch.float64)
    lp = lp.to(DEV)
    s, d, _ = dv.run(False, logp_old=lp)
    s_z, d_z, _ = dv.run(False, logp_old=lp, pi_coef=0.0)
    assert bool(torch.isfinite(d[rows]).all())
    assert torch.equal(d[rows], d_z[rows])
    assert not torch.equal(d[:N], d_z[:N])                          # (the other rows do have a policy part)
    _, _, keep = ops.ppo_rows_host(c["rec64"]["logp"][:N].numpy(), lp.cpu().numpy(), c["advs"].double().numpy(), CLIP)
    assert not keep[rows].any() and float(s[3]) == float((~keep).sum())
    assert np.isfinite(float(s[0])) and not np.isfinite(float(s[4]))      # the surrogate is the clipped branch; KL is not finite


@pytest.mark.parametrize("kind,n", [("d", 6), ("g", 3)])
def test_two_shares_equal_the_one_shot_run(kind, n):
    N, n1 = 1000, 400
    c = case(kind, N, n, True)
    dv = Dev(c)
    for record in (True, False):
        def lp_buf():
            return None if record else torch.cat([c["logp_old"], torch.full((2,), SENT, dtype=torch.float64)]).to(DEV)
        s_all, d_all, lp_all = dv.run(record, logp_old=lp_buf())
        s_a, d_a, lp_a = dv.run(record, logp_old=lp_buf(), lo=0, hi=n1)
        s_b, d_b, lp_b = dv.run(record, logp_old=lp_buf(), lo=n1, hi=N)
        assert dv.guards_intact(d_a, lp_a if record else None, 0, n1) and dv.guards_intact(d_b, lp_b if record else None, n1, N)
        assert torch.equal(d_a[:n1], d_all[:n1]) and torch.equal(d_b[n1:N], d_all[n1:N])
        assert torch.equal(lp_a[:n1], lp_all[:n1]) and torch.equal(lp_b[n1:N], lp_all[n1:N])
        np.testing.assert_allclose((s_a + s_b).numpy(), s_all.numpy(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("kind,n", [("d", 6), ("g", 3)])
def test_argument_checks_leave_the_outputs_untouched(kind, n):
    c = case(kind, 255, n, False)
    dv = Dev(c)
    N, W = c["N"], dv.W
    db = torch.full((N, W + 2), SENT, device=DEV)
    lp = torch.full((N,), SENT, dtype=torch.float64, device=DEV)
    s = torch.full((5,), 5.0, dtype=torch.float64, device=DEV)
    fn = ops.ppo_loss_fwd_bwd if kind == "d" else ops.gauss_ppo_fwd_bwd
    acts = dv.acts if kind == "d" else dv.acts[:, :n]

    def call(rows=N, clip=CLIP, record=1, n_global=N, n_arg=n, asum=None, x=None):
        x = dv.hb[:, :W] if x is None else x
        head = (x[:rows], dv.hb[:rows, W], acts[:rows], dv.advs[:rows], dv.rets[:rows], asum, n_global)
        if kind == "g":
            head += (n_arg,)
        # (an empty view's data_ptr() is NULL: logp_old keeps its address when there are no rows)
        fn(*head, PC, VC, EC, clip, record, lp[:rows] if rows else lp, db[:rows, :W], db[:rows, W], s)
    asum = torch.tensor([1.0, 2.0], dtype=torch.float64, device=DEV)
    bad = [dict(clip=0.0), dict(clip=-0.2), dict(clip=float("inf")), dict(clip=float("nan")), dict(record=2), dict(record=-1),
           dict(n_global=N - 1), dict(rows=1, n_global=1, asum=asum)]
    if kind == "d":
        bad.append(dict(x=torch.zeros(N, 33, device=DEV)))
    else:
        bad += [dict(n_arg=0), dict(n_arg=65), dict(x=dv.hb[:, :W - 1].contiguous())]
    for kw in bad:
        with pytest.raises(A2CKernelError):
            call(**kw)
    st = ops.stream()
    scratch = ops.reduce_scratch(dv.hb.device, st)
    name = "a2c_ppo_loss_fwd_bwd" if kind == "d" else "a2c_gauss_ppo_fwd_bwd"
    P = lambda t: t.data_ptr()
    for null in ("logp_old", "grad"):       # a NULL logp_old, a NULL gradient array
        lp_p, db_p = (None, P(db)) if null == "logp_old" else (P(lp), None)
        if kind == "d":
            rc = getattr(ops.lib(), name)(P(dv.hb), W + 2, P(dv.hb[:, W]), W + 2, P(acts), P(dv.advs), P(dv.rets), None, N, N,
                                          n, PC, VC, EC, CLIP, 1, lp_p, db_p, W + 2, P(db[:, W]), W + 2, P(s), P(scratch), st)
        else:
            rc = getattr(ops.lib(), name)(P(dv.hb), W + 2, P(dv.hb[:, W]), W + 2, P(dv.acts), n + 1, P(dv.advs), P(dv.rets), None,
                                          N, N, n, PC, VC, EC, CLIP, 1, lp_p, db_p, W + 2, P(db[:, W]), W + 2, P(s), P(scratch), st)
        with pytest.raises(A2CKernelError):
            ops.check(rc, name)
    torch.cuda.synchronize()
    assert bool((db == SENT).all()) and bool((lp == SENT).all()) and bool((s == 5.0).all())
    call(rows=0)                            # n_local = 0 zeroes the five sums and writes nothing else
    torch.cuda.synchronize()
    assert bool((s == 0.0).all()) and bool((db == SENT).all()) and bool((lp == SENT).all())


# ------------------------------------------------------------------------------------- 2. K epochs against fp64
K_EPOCHS = 3
# seed and ppo_clip of each case: chosen with the float64 restatement alone, so that no row's ratio comes within 1e-3 of an
# edge in epochs 1 .. K-1 and the clip stops at least two rows in the last epoch (the test asserts both)
UPDATE_CASES = [  # name, kind, discrete, n (actions / action dims), use_bptt, optim, lr, norm_advs, seed, ppo_clip
    ("fc_discrete_sgd", "FCModel", True, 4, False, "SGD", 0.1, True, 3102, 0.02),
    ("fc_n3_sgd", "FCModel", False, 3, False, "SGD", 0.1, False, 2110, 0.02),
    ("fc_n3_rms", "FCModel", False, 3, False, "RMSprop", 1e-4, True, 2110, 0.2),
    ("grufc_n2_sgd", "GRUFCModel", False, 2, False, "SGD", 0.1, True, 2122, 0.2),
    ("grufc_bptt_n1_sgd", "GRUFCModel", False, 1, True, "SGD", 0.1, False, 2130, 0.2),
]


def update_case(case, **kw):
    """-> (state dict, hyps, host shared data) of one case"""
    name, kind, discrete, n, use_bptt, opt, lr, norm, seed, clip = case
    recurrent = kind == "GRUFCModel"
    D = CC.synth_shared(n, UPDATE_H, UPDATE_R, UPDATE_T, seed=seed, recurrent=recurrent)
    common = dict(n_tsteps=UPDATE_T, n_rollouts=UPDATE_R, optim_type=opt, lr=lr, norm_advs=norm, use_bptt=use_bptt,
                  h_size=UPDATE_H, ppo_epochs=K_EPOCHS, ppo_clip=clip)
    if discrete:
        sd = O.formula_state_dict(kind, CC.STATE_SHAPE, n, UPDATE_H)
        hyps = base_hyps(n_frame_stack=CC.C_STACK, env_type="ContEnv", **common)
        D["actions"] = torch.from_numpy(np.minimum(hashf(UPDATE_R * UPDATE_T, seed + 3, 0, n).astype(np.int64), n - 1))
    else:
        sd = CC.state_dict(kind, n, UPDATE_H, RAW_BIAS[n])
        hyps = CC.cont_hyps(gauss_loss="exact", **common)
    hyps.update(kw)
    return sd, hyps, D


def ppo_update64(kind, sd, discrete, n, hyps, D, use_bptt, dtype=torch.float64):
    """one update of K epochs restated: forward (flat, recurrent-flat or stepped over time with the done reset), the clipped
    loss with logp_old detached from epoch 0, clip_grad_norm_, torch.optim, K times on the same advantages and returns
    -> (info of the last epoch, parameters by name, the smallest distance of any row's ratio from 1 +- clip in epochs
    1 .. K-1, the number of rows the clip stops in the last epoch)"""
    P, rows = net64(kind, sd, dtype)
    params = list(P.values())
    opt = getattr(torch.optim, hyps["optim_type"])(params, lr=hyps["lr"])
    R_, T, K, clip = hyps["n_rollouts"], hyps["n_tsteps"], hyps["ppo_epochs"], hyps["ppo_clip"]
    S, dn = D["states"].to(dtype), D["dones"].double()
    advs = scan64(D["deltas"].double(), dn, hyps["gamma"] * hyps["lambda_"]).to(dtype)
    rets = scan64(D["rewards"].double(), dn, hyps["gamma"]).to(dtype)
    w = (advs - advs.mean()) / (advs.std() + 1e-6) if hyps["norm_advs"] else advs
    acts = D["actions"] if discrete else D["actions"].to(dtype)
    A = n if discrete else 2 * n
    logp_old, margin = None, float("inf")
    for epoch in range(K):
        if use_bptt:
            hs = D["h_states"].to(dtype).view(R_, T, -1)[:, 0]
            alive = (1 - dn.to(dtype)).view(R_, T, 1)
            outs = []
            for t in range(T):
                o, hs = rows(S.view(R_, T, *S.shape[1:])[:, t], hs)
                hs = hs * alive[:, t]
                outs.append(o)
            heads = torch.stack(outs, dim=1).reshape(R_ * T, -1)
        else:
            heads = rows(S, D["h_states"].to(dtype) if kind == "GRUFCModel" else None)[0]
        logp, neg_h = policy_rows("d" if discrete else "g", heads[:, :A], acts, n)
        if epoch == 0:
            logp_old = logp.detach().clone()
        r, surr, keep = ppo_terms(logp, logp_old, w, clip)
        pi = -hyps["pi_coef"] * surr.mean()
        vl = hyps["val_coef"] * ((heads[:, A] - rets) ** 2).mean()
        en = -hyps["entr_coef"] * neg_h.mean()
        loss = pi + vl - en
        opt.zero_grad()
        loss.backward()
        gnorm = torch.nn.utils.clip_grad_norm_(params, hyps["max_norm"])
        opt.step()
        rd = r.detach()
        if epoch:
            margin = min(margin, float(torch.minimum((rd - (1 + clip)).abs(), (rd - (1 - clip)).abs()).min()))
    info = {"Loss": float(loss.detach()), "Pi_Loss": float(pi.detach()), "ValLoss": float(vl.detach()), "Entropy": float(en.detach()),
            "GradNorm": float(gnorm)}
    extra = {"ClipFrac": float((~keep).sum()) / len(rd), "ApproxKL": float(((rd - 1) - rd.log()).mean())}
    return info, {k: v.detach().double() for k, v in P.items()}, margin, int((~keep).sum()), extra


def _gpu_net(kind, discrete, n, sd):
    net = getattr(a2c_amd, kind)(list(CC.STATE_SHAPE), n, h_size=UPDATE_H, **({} if discrete else dict(is_discrete=False)))
    net.load_state_dict(sd)
    return net.cuda()


@pytest.mark.parametrize("case", UPDATE_CASES, ids=[c[0] for c in UPDATE_CASES])
def test_k_epochs_match_the_fp64_restatement(case):
    """the bound is K times the one-update bounds of test_gpu_gauss_exact.py: each of the K steps contributes at most one
    such error to first order"""
    name, kind, discrete, n, use_bptt = case[:5]
    sd, hyps, D = update_case(case)
    want_info, want_P, margin, n_clipped, extra = ppo_update64(kind, sd, discrete, n, hyps, D, use_bptt)
    print(f"{name}: smallest |r - (1 +- clip)| in epochs 1.. {margin:.3e}, rows clipped in the last epoch {n_clipped}")
    assert margin >= 1e-3 and n_clipped >= 2            # conditions on the inputs: no ratio near an edge, the clip bites
    net = _gpu_net(kind, discrete, n, sd)
    upd = Updater(net, hyps)
    info = upd.update_model({k: v.cuda() for k, v in D.items()})
    got_P = {k: p.detach().cpu() for k, p in net.named_parameters()}
    assert sorted(got_P) == sorted(want_P) and sorted(info) == sorted({**want_info, **extra})
    ri, rp = info_bound_ratio(info, want_info), param_bound_ratio(got_P, want_P)
    moved = max(float((want_P[k] - sd[k].double()).abs().max()) for k in want_P)
    print(f"{name}: info error / bound {ri:.4f}, parameter error / bound {rp:.4f} (allowed {K_EPOCHS}), largest parameter step "
          f"{moved:.3e}", info, extra)
    assert moved > 1e-4
    assert ri <= K_EPOCHS, (info, want_info)
    assert rp <= K_EPOCHS
    assert info["ClipFrac"] == extra["ClipFrac"] == n_clipped / (UPDATE_R * UPDATE_T)
    assert abs(info["ApproxKL"] - extra["ApproxKL"]) <= 1e-6 + 1e-4 * abs(extra["ApproxKL"]), (info, extra)
    assert upd.optim._steps == K_EPOCHS


# ------------------------------------------------------------------------------- 3. one epoch is today's update
def _run_update(case, updates=1, **kw):
    name, kind, discrete, n = case[:4]
    sd, hyps, D = update_case(case, **kw)
    for k, v in kw.items():
        if v is None:
            del hyps[k]
    net = _gpu_net(kind, discrete, n, sd)
    upd = Updater(net, hyps)
    Dd = {k: v.cuda() for k, v in D.items()}
    infos = [dict(upd.update_model(Dd)) for _ in range(updates)]
    return infos, torch.cat([p.detach().reshape(-1) for p in net.parameters()]), upd


def _ppo_counts():
    by = ops.torch_abi().stats["by_name"]
    return {k: v for k, v in by.items() if "ppo" in k}


@pytest.mark.parametrize("case", [UPDATE_CASES[0], UPDATE_CASES[2]], ids=lambda c: c[0])
def test_one_epoch_is_the_update_without_the_keys(case, monkeypatch):
    i0, p0, u0 = _run_update(case, updates=2, ppo_epochs=None, ppo_clip=None)
    assert "ppo_epochs" not in u0.hyps and "ppo_clip" not in u0.hyps
    i1, p1, u1 = _run_update(case, updates=2, ppo_epochs=1, ppo_clip=0.3)
    assert torch.equal(p0, p1) and i0 == i1 and all(len(i) == 5 for i in i1)
    assert "logp_old" not in u1._bufs and "ppo_sums" not in u1._bufs
    monkeypatch.setenv("A2C_TORCH_OPS", "1")
    if not os.path.exists(os.path.join(os.path.dirname(ops.__file__), "liba2c_torch_ops.so")):
        pytest.fail("liba2c_torch_ops.so was not built")
    before = _ppo_counts()
    i2, p2, _ = _run_update(case, updates=2, ppo_epochs=1, ppo_clip=0.3)
    assert _ppo_counts() == before, "a ppo launch with ppo_epochs = 1"
    assert torch.equal(p0, p2) and i0 == i2


@pytest.mark.parametrize("case", [UPDATE_CASES[0], UPDATE_CASES[2]], ids=lambda c: c[0])
def test_torch_ops_path_is_bit_identical(case, monkeypatch):
    i0, p0, _ = _run_update(case, updates=2)
    monkeypatch.setenv("A2C_TORCH_OPS", "1")
    if not os.path.exists(os.path.join(os.path.dirname(ops.__file__), "liba2c_torch_ops.so")):
        pytest.fail("liba2c_torch_ops.so was not built")
    name, sibling = ("a2c_ppo_loss_fwd_bwd", "a2c_loss_fwd_bwd") if case[2] else ("a2c_gauss_ppo_fwd_bwd", "a2c_gauss_nll_fwd_bwd")
    assert hasattr(torch.ops.a2c_mi355x, "abi_" + name[4:])
    before = dict(ops.torch_abi().stats["by_name"])
    i1, p1, _ = _run_update(case, updates=2)
    after = ops.torch_abi().stats["by_name"]
    assert after.get(name, 0) - before.get(name, 0) == 2 * K_EPOCHS, after          # K launches an update
    assert after.get(sibling, 0) == before.get(sibling, 0), after
    assert torch.equal(p0, p1) and i0 == i1
    assert all(len(i) == 7 for i in i1)


# --------------------------------------------------------------------------------------- 4. captured equals eager
GRAPH_CASES = [("fc_rms", UPDATE_CASES[2], {}), ("grufc_bptt_rms", UPDATE_CASES[4], dict(optim_type="RMSprop", lr=1e-4)),
               ("fc_adam_capturable", UPDATE_CASES[2], dict(optim_type="Adam", lr=1e-4, optim_capturable=True))]


@pytest.mark.parametrize("name,case,kw", GRAPH_CASES, ids=[g[0] for g in GRAPH_CASES])
def test_graphed_update_equals_eager(name, case, kw):
    def run(graphed):
        _, kind, discrete, n = case[:4]
        sd, hyps, D = update_case(case, **kw)
        net = _gpu_net(kind, discrete, n, sd)
        upd = Updater(net, hyps)
        Dd = {k: v.cuda() for k, v in D.items()}
        infos = [dict(upd.update_model(Dd))]
        if graphed:
            rep = upd.capture_update(Dd)
            assert len(rep.graphs) == 1                  # the K epochs are one graph
            infos += [dict(rep()), dict(rep())]
        else:
            infos += [dict(upd.update_model(Dd)), dict(upd.update_model(Dd))]
        steps = {float(s["step"]) for s in upd.optim.state_dict()["state"].values()}
        return infos, torch.cat([p.detach().reshape(-1) for p in net.parameters()]), steps, upd.optim._steps
    ie, pe, se, ne = run(False)
    ig, pg, sg, ng = run(True)
    assert torch.equal(pe, pg)
    assert ie == ig and all(len(i) == 7 for i in ig)
    assert len({i["Loss"] for i in ig}) == 3                 # the replays did step
    assert ne == ng == 3 * K_EPOCHS and se == sg == {float(3 * K_EPOCHS)}      # K optimiser steps an update


# ------------------------------------------------------------------------------------------------ 5. the refusals
class _ActiveShard:
    """what Updater.__init__ reads of a parallel.Shard that spans two ranks"""
    active, rank, world, group = True, 0, 2, None


def test_refusals_name_the_key_before_any_device_work():
    sd, hyps, D = update_case(UPDATE_CASES[2])
    net = _gpu_net("FCModel", False, 3, sd)
    for kw, key in ((dict(gauss_loss="reference"), "ppo_epochs"), (dict(ppo_epochs=0), "ppo_epochs"),
                    (dict(ppo_epochs=2.0), "ppo_epochs"), (dict(ppo_epochs="3"), "ppo_epochs"), (dict(ppo_clip=0.0), "ppo_clip"),
                    (dict(ppo_clip=-1.0), "ppo_clip"), (dict(ppo_clip=float("nan")), "ppo_clip"),
                    (dict(ppo_clip=float("inf")), "ppo_clip")):
        with pytest.raises(ValueError, match=key):
            Updater(net, dict(hyps, **kw))
    with pytest.raises(ValueError, match="ppo_epochs"):
        Updater(net, hyps, shard=_ActiveShard())
    Updater(net, dict(hyps, ppo_epochs=1), shard=None)
    a3c = a2c_amd.A3CModel([4, 84, 84], 3, h_size=32).cuda()
    with pytest.raises(ValueError, match="ppo_epochs"):
        Updater(a3c, base_hyps(ppo_epochs=2))
    Updater(a3c, base_hyps(ppo_epochs=1))


# ------------------------------------------------------------------------------------------------ 6. it learns
def _bandit(n, seed, **kw):
    """the one-state bandit of tests/test_gpu_gauss_exact.py: same rows, seeds, optimiser and 60 updates -> (start, end, info)"""
    torch.manual_seed(seed)
    net = a2c_amd.FCModel([1, 1, 8], n, h_size=32, is_discrete=False).cuda()
    upd = Updater(net, bandit_hyps(gauss_loss="exact", **kw))
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
    return start, miss(), info


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 2])
def test_bandit_mu_moves_to_the_rewarded_action_with_four_epochs(n, seed):
    """the bar of test_gpu_gauss_exact.py: 60 updates of 256 sampled rows bring |mu - 1.5| to at most a quarter of where it
    started, here with ppo_epochs = 4, ppo_clip = 0.2 (K = 1 printed beside it)"""
    s1, e1, _ = _bandit(n, seed)
    s4, e4, info = _bandit(n, seed, ppo_epochs=4, ppo_clip=0.2)
    print(f"n={n} seed={seed}: |mu - 1.5| K=1 {s1:.4f} -> {e1:.4f} ({e1 / s1:.4f} of the start), K=4 {s4:.4f} -> {e4:.4f} "
          f"({e4 / s4:.4f} of the start)", info)
    assert all(np.isfinite(x) for x in info.values()), info
    assert e4 <= 0.25 * s4, (s4, e4)
