"""-m gpu: the small kernels between the matrix products of every update and rollout step -- the A2C loss, the Gaussian
loss, the GRU gate math and the two-launch GRU cell, LayerNorm, the advantage statistics, the samplers, the column
sums, the composed head, the split-K slabs and the bit unpacker -- called through the C ABI (a2c_amd.ops) and compared
with an fp64 evaluation of the reference's formula on the CPU.

The criterion is the one of the optimiser tests (`_crit`): e_k = max|kernel - fp64| <= 2 e_t + ulp, with e_t =
max|fp32 torch on the CPU - fp64| for the same formula and ulp one fp32 ulp at the magnitude of the largest term summed
into an element of that array (stated at every call).  Where a case is too small for e_t to mean anything (one element
of torch's run is often exact by chance) the two torch runs also cover a pool of further rows of the same distribution
that the kernel does not see.  Integer outputs and outputs documented as bit-identical to another path are exact.  The
fp64 loss sums are held to n rows times the per-row bound.

Long sums (a2c_colsum, the split-K slabs) take e_t from the plain fp32 running sum in index order (`_running_sum`), not
from Tensor.sum / mm: torch's CPU reductions cascade their partial sums, an advantage no fixed-order fp32 sum shares;
against Tensor.sum the column sums measured 1.9 - 5.5 x e_t at 300 - 32 768 rows, the slabs 2.5 - 10 x at K = 4104.  That
difference is charged to torch.  With A2C_GRU_K4=1 the cell kernels are compared bit for bit with the five launches
wherever a2c_gemm_f32 runs those on its four-wave small-product kernel (`five_launches_comparable`).

Worst e_k / e_t per array measured on an MI355X over all cases of this file (`pytest -s` prints them at the end):
loss dlogits 2.87 (inside the bound by the ulp of its largest term), dvals 1.00; Gaussian dheads 1.00; gru_gates z, r,
rh 1.00; gru_out c 1.39, h_new 1.00; gru_out_bwd, gru_out_bwd_carry, gru_gates_bwd 1.00 throughout; gru_cell_fwd
(eight-way split) gx 1.04, z 1.00, r 1.10, rh 1.02, c 0.96, h_new 1.00, (four-way) the same but h_new 1.04; gru_cell_bwd
dc_pre, dz, dz_pre 1.00, dr_pre 0.60 (four-way 0.95), dh 0.97; LayerNorm mean 11.9 (torch's cascaded mean is nearly
exact; the kernel's is within the ulp of max|x|), rstd 1.00, y 1.67, dx 1.48, dw_rows 1.76, their column sum 1.00;
normalize 1.00; softmax_sample's probabilities 2.12; colsum 1.00 and the split-K slabs 1.04 (against the running sum);
compose_heads Wc 1.00, bc 1.59.  The moments are within 1.5e-16 relative of math.fsum.  Wall time of the file
inside a run of the whole suite: 5.1 s of test calls (test_gpu_optimizers.py: 7.8 s); 13 s on its own.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import a2c_oracle as O  # noqa: E402
from test_gpu_continuous import _rand_heads, _reference_loss  # noqa: E402

DEV = "cuda"
ERR_ARG, ERR_WORKSPACE = -1, -3
SENT = 12345.6787109375            # sentinel value (an exact float32) of every padded output
POOL = 512                         # rows of the two torch runs where the kernel sees fewer

_RATIOS = {}


def _ops():
    from a2c_amd import ops
    return ops


def _err():
    from a2c_amd import _lib
    return _lib.A2CKernelError


def _raises(code, fn, *a, **kw):
    with pytest.raises(_err()) as ei:
        fn(*a, **kw)
    assert f"(code {code})" in str(ei.value), str(ei.value)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _u(shape, seed, lo=-1.0, hi=1.0):
    """uniform at full fp32 resolution"""
    return (torch.rand(shape, generator=_gen(seed), dtype=torch.float64) * (hi - lo) + lo).float()


def _nrm(shape, seed):
    return torch.randn(shape, generator=_gen(seed))


def _crit(tag, got, t32, t64, scale=None):
    """e_k <= 2 e_t + ulp(scale).  `got` may be the leading part (rows) of what the two torch runs cover.  scale: the
    magnitude of the largest term summed into an element; default max|fp64| (an array whose elements are single
    products or function values).  -> e_k / e_t"""
    t64 = t64.detach().double().reshape(-1)
    t32 = t32.detach().double().reshape(-1)
    g = got.detach().cpu().double().reshape(-1)
    n = g.numel()
    assert n <= t64.numel() and t32.numel() == t64.numel(), (tag, n, t32.numel(), t64.numel())
    if n == 0:
        return None
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


def _running_sum(x, dim=0):
    """the plain fp32 running sum in index order along `dim`, every addition rounded to fp32.  e_t of a long sum is taken
    from this and not from Tensor.sum / mm: torch's CPU reductions cascade (several levels of partial sums, error
    O(log n)), a rounding advantage no fixed-order fp32 sum on the GPU shares; that difference is charged to torch.
    (Tensor.cumsum is no substitute: on the CPU it accumulates floats in double.)"""
    x = x.movedim(dim, 0)
    s = torch.zeros_like(x[0])
    for i in range(x.shape[0]):
        s += x[i]
    return s


def _running_mm(a, b):
    """a @ b with the same plain running sum over k (products and additions each rounded to fp32)"""
    s = torch.zeros(a.shape[0], b.shape[1], dtype=a.dtype)
    for k in range(a.shape[1]):
        s += a[:, k, None] * b[None, k, :]
    return s


def _sent(*shape):
    return torch.full(shape, SENT, device=DEV)


def _is_sent(t):
    return bool((t == SENT).all())


# ====================================================================================================== loss
PC, VC, EC = 0.8, 0.5, 0.01
GAP = 120.0          # expf(-120) = 0 in fp32 (the smallest subnormal is 1.4e-45 = exp(-103.3))


def _loss_inputs(N, A, seed):
    """Np = max(N, POOL) rows; every tenth row or so has one logit GAP above the rest (half of them act on it, half on
    another), another tenth has all logits equal, and a seventh of the actions are -1"""
    Np = max(N, POOL)
    g = _gen(seed)
    lg = (torch.rand(Np, A, generator=g, dtype=torch.float64) * 6 - 3).float()
    kind = torch.randint(0, 10, (Np,), generator=g)
    acts = torch.randint(0, A, (Np,), generator=g)
    dom = torch.randint(0, A, (Np,), generator=g)
    rows = (kind == 0).nonzero().flatten()
    lg[rows, dom[rows]] += GAP
    half = rows[::2]
    acts[half] = dom[half]
    lg[kind == 1] = 0.5
    acts[torch.randint(0, 7, (Np,), generator=g) == 0] = -1
    v = _nrm((Np,), seed + 1)
    advs = _nrm((Np,), seed + 2) * 1.5 + 0.3
    rets = _nrm((Np,), seed + 3)
    return lg, v, acts, advs, rets, kind


def _loss_ref(lg, v, acts, advs, rets, NG, norm, dtype):
    """updater.py:97-98, 100-106, 124-127 over the first NG rows as the batch (means are sums / NG); rows past NG are the
    pool: same statistics, same 1 / NG"""
    lg = lg.to(dtype).clone().requires_grad_(True)
    v = v.to(dtype).clone().requires_grad_(True)
    a = advs.to(dtype)
    if norm:
        a = (a - a[:NG].mean()) / (a[:NG].std() + 1e-6)
    lsm = F.log_softmax(lg, dim=-1)
    t_pi = lsm[torch.arange(len(acts)), acts] * a
    t_ent = (lsm * F.softmax(lg, dim=-1)).sum(-1)
    t_val = (v - rets.to(dtype)) ** 2
    loss = PC * -(t_pi.sum() / NG) + VC * (t_val.sum() / NG) + EC * (t_ent.sum() / NG)
    loss.backward()
    return dict(t_pi=t_pi.detach(), t_val=t_val.detach(), t_ent=t_ent.detach(), dl=lg.grad, dv=v.grad, a=a.detach(),
                lsm=lsm.detach())


def _dlogit_scale(r64, acts, NG):
    """largest of the two terms of a dlogits element: pi_coef adv / N (1[j == act] - p_j) and entr_coef / N p_j (lsm_j - plp)"""
    lsm = r64["lsm"]
    p = lsm.exp()
    A = lsm.shape[1]
    onehot = F.one_hot(torch.where(acts < 0, acts + A, acts), A).double()
    ta = (PC * r64["a"].abs() / NG)[:, None] * (onehot - p).abs()
    tb = EC / NG * (p * (lsm - r64["t_ent"][:, None])).abs()
    return max(float(ta.max()), float(tb.max()))


def _layout(lg, v, layout, extra=2):
    """device heads buffer with the logits and the value as column slices, and the twin for the gradients full of sentinels;
    'heads': rows [logits | value] (stride A + 1, the Updater's), 'wide': [x | logits | x | value | x], 'packed': own arrays"""
    N, A = lg.shape
    if layout == "packed":
        dl = _sent(N + extra, A)
        dv = _sent(N + extra)
        return lg.to(DEV).contiguous(), v.to(DEV).contiguous(), dl[:N], dv[:N], (dl, dv), None
    W, c0, cv = (A + 1, 0, A) if layout == "heads" else (A + 4, 1, A + 2)
    hb = _sent(N + extra, W)
    hb[:N, c0:c0 + A] = lg.to(DEV)
    hb[:N, cv] = v.to(DEV)
    db = _sent(N + extra, W)
    keep = torch.ones(N + extra, W, dtype=torch.bool, device=DEV)
    keep[:N, c0:c0 + A] = False
    keep[:N, cv] = False
    return hb[:N, c0:c0 + A], hb[:N, cv], db[:N, c0:c0 + A], db[:N, cv], (db,), keep


def _check_sentinels(bufs, keep, N):
    if keep is None:
        dl, dv = bufs
        assert _is_sent(dl[N:]) and _is_sent(dv[N:])
    else:
        assert _is_sent(bufs[0][keep]), "a sentinel beside / behind the gradients was overwritten"


def _adv_sums(advs_dev):
    s = torch.zeros(2, dtype=torch.float64, device=DEV)
    _ops().moments(advs_dev.contiguous(), s)
    return s


def _check_loss_sums(tag, s, r32, r64, n, rows=slice(None)):
    """the three fp64 sums against the fp64 sum of the per-row terms; every row's term is allowed 2 e_t + ulp (e_t of the
    fp32 per-row terms, ulp at the largest term), the sum n times that: the summation itself is in fp64 and adds nothing"""
    for i, k in enumerate(("t_pi", "t_val", "t_ent")):
        t64, t32 = r64[k][rows].double(), r32[k][rows].double()
        e_t = float((r32[k].double() - r64[k]).abs().max())
        ulp = float(np.spacing(np.float32(r64[k].abs().max())))
        want, s32 = float(t64.sum()), float(t32.sum())
        e_k = abs(float(s[i]) - want)
        print(f"    {tag} sum {k}: |kernel - fp64| {e_k:.3e}, |sum of fp32 terms - fp64| {abs(s32 - want):.3e}, "
              f"bound {n * (2 * e_t + ulp):.3e}")
        assert e_k <= n * (2 * e_t + ulp), (tag, k, float(s[i]), want)


LOSS_A = [1, 2, 3, 6, 18, 32]
LOSS_N = [1, 2, 255, 256, 257, 32768, 300007]      # 300 007 > 1024 * 256: rows revisited by grid-stride
LOSS_CASES = [(A, N, norm) for A in LOSS_A for N in LOSS_N for norm in (False, True) if not (norm and N < 2)]


@pytest.mark.parametrize("A,N,norm", LOSS_CASES)
def test_loss_fwd_bwd_vs_fp64(A, N, norm):
    """a2c_loss_fwd_bwd (updater.py:100-106, 124-127) at every A up to MAXA and N from one row to the grid-stride path, with
    -1 actions, underflowing probabilities, all-equal logits, the three buffer layouts and sentinels around the outputs;
    twice: identical sums"""
    ops = _ops()
    lg, v, acts, advs, rets, kind = _loss_inputs(N, A, 1000 + 37 * A + N % 997)
    if N >= 255:
        assert (kind[:N] == 0).any() and (kind[:N] == 1).any() and (acts[:N] == -1).any()
    r64 = _loss_ref(lg, v, acts, advs, rets, N, norm, torch.float64)
    r32 = _loss_ref(lg, v, acts, advs, rets, N, norm, torch.float32)
    layout = ("heads", "wide", "packed")[(A + N + int(norm)) % 3]
    lgd, vd, dl, dv, bufs, keep = _layout(lg[:N], v[:N], layout)
    ad, rd, actd = advs[:N].to(DEV), rets[:N].to(DEV), acts[:N].to(DEV)
    asum = _adv_sums(ad) if norm else None
    sums = []
    for _ in range(2):
        s = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
        ops.loss_fwd_bwd(lgd, vd, actd, ad, rd, asum, N, PC, VC, EC, dl, dv, s)
        sums.append(s.cpu())
    assert torch.equal(sums[0], sums[1]), "the loss sums differ between two identical calls"
    _check_sentinels(bufs, keep, N)
    _crit("loss.dlogits", dl, r32["dl"], r64["dl"], _dlogit_scale(r64, acts, N))
    _crit("loss.dvals", dv, r32["dv"], r64["dv"])
    _check_loss_sums("loss", sums[0], r32, r64, N, slice(0, N))


@pytest.mark.parametrize("A,N", [(3, 2), (6, 257), (18, 5000)])
def test_loss_constant_advantages_normalised(A, N):
    """a constant advantage vector with normalisation on: the variance clamps to 0, den = 1e-6 and every normalised
    advantage is 0 (0.75 and its sums are exact in fp32, so the torch runs say the same); only the entropy term is left"""
    ops = _ops()
    lg, v, acts, _, rets, _ = _loss_inputs(N, A, 77 + A)
    advs = torch.full((max(N, POOL),), 0.75)
    r64 = _loss_ref(lg, v, acts, advs, rets, N, True, torch.float64)
    r32 = _loss_ref(lg, v, acts, advs, rets, N, True, torch.float32)
    assert float(r64["a"].abs().max()) == 0.0
    lgd, vd, dl, dv, bufs, keep = _layout(lg[:N], v[:N], "heads")
    ad = advs[:N].to(DEV)
    s = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    ops.loss_fwd_bwd(lgd, vd, acts[:N].to(DEV), ad, rets[:N].to(DEV), _adv_sums(ad), N, PC, VC, EC, dl, dv, s)
    _check_sentinels(bufs, keep, N)
    assert float(s[0]) == 0.0
    _crit("loss.dlogits const-adv", dl, r32["dl"], r64["dl"], _dlogit_scale(r64, acts, N))
    _check_loss_sums("loss const-adv", s.cpu(), r32, r64, N, slice(0, N))


@pytest.mark.parametrize("A,N,n1,norm", [(6, 1000, 300, True), (3, 300007, 100000, True), (18, 513, 512, False), (2, 2, 1, True)])
def test_loss_two_shards_of_one_batch(A, N, n1, norm):
    """two ranks' shards (n_local < n_global, the common all-reduced adv_sums): the three sums add up to the one-call sums
    within the criterion, the gradient rows are the one-call rows bit for bit"""
    ops = _ops()
    lg, v, acts, advs, rets, _ = _loss_inputs(N, A, 555 + A)
    r64 = _loss_ref(lg, v, acts, advs, rets, N, norm, torch.float64)
    r32 = _loss_ref(lg, v, acts, advs, rets, N, norm, torch.float32)
    ad, rd, actd = advs[:N].to(DEV), rets[:N].to(DEV), acts[:N].to(DEV)
    asum = _adv_sums(ad) if norm else None
    lgd, vd, dl, dv, _, _ = _layout(lg[:N], v[:N], "heads")
    s_all = torch.zeros(3, dtype=torch.float64, device=DEV)
    ops.loss_fwd_bwd(lgd, vd, actd, ad, rd, asum, N, PC, VC, EC, dl, dv, s_all)
    lg2, v2, dl2, dv2, bufs2, keep2 = _layout(lg[:N], v[:N], "heads")
    parts = []
    for lo, hi in ((0, n1), (n1, N)):
        s = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
        ops.loss_fwd_bwd(lg2[lo:hi], v2[lo:hi], actd[lo:hi], ad[lo:hi], rd[lo:hi], asum, N, PC, VC, EC, dl2[lo:hi],
                         dv2[lo:hi], s)
        parts.append(s.cpu())
        _check_loss_sums(f"loss shard {lo}:{hi}", s.cpu(), r32, r64, hi - lo, slice(lo, hi))
    _check_sentinels(bufs2, keep2, N)
    assert torch.equal(dl2, dl) and torch.equal(dv2, dv), "a shard's gradient rows differ from the one-call rows"
    _check_loss_sums("loss shards added", parts[0] + parts[1], r32, r64, N, slice(0, N))
    # the same fp32 terms in another fp64 order: N * 2^-53 of the sum of their magnitudes
    for i, k in enumerate(("t_pi", "t_val", "t_ent")):
        tol = 4 * N * 2.0 ** -53 * float(r32[k][:N].double().abs().sum())
        assert abs(float(parts[0][i] + parts[1][i]) - float(s_all[i])) <= tol, (k, parts, s_all)


def test_loss_argument_errors_launch_nothing():
    ops = _ops()
    N = 64
    mk = lambda A: (torch.zeros(N, A, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, dtype=torch.int64, device=DEV),
                    torch.ones(N, device=DEV), torch.zeros(N, device=DEV), _sent(N, A), _sent(N))
    s = torch.full((3,), 7.0, dtype=torch.float64, device=DEV)
    asum = torch.tensor([1.0, 2.0], dtype=torch.float64, device=DEV)
    lg, v, a, ad, r, dl, dv = mk(33)
    _raises(ERR_ARG, ops.loss_fwd_bwd, lg, v, a, ad, r, None, N, PC, VC, EC, dl, dv, s)            # A = 33 > MAXA
    assert _is_sent(dl) and _is_sent(dv)
    lg, v, a, ad, r, dl, dv = mk(4)
    _raises(ERR_ARG, ops.loss_fwd_bwd, lg, v, a, ad, r, None, N - 1, PC, VC, EC, dl, dv, s)        # n_global < n_local
    _raises(ERR_ARG, ops.loss_fwd_bwd, lg[:1], v[:1], a[:1], ad[:1], r[:1], asum, 1, PC, VC, EC, dl[:1], dv[:1], s)
    torch.cuda.synchronize()
    assert _is_sent(dl) and _is_sent(dv) and bool((s == 7.0).all())
    ops.loss_fwd_bwd(lg[:0], v[:0], a[:0], ad[:0], r[:0], asum, N, PC, VC, EC, dl[:0], dv[:0], s)   # n_local = 0
    assert bool((s == 0.0).all()) and _is_sent(dl) and _is_sent(dv)


# ====================================================================================================== Gaussian loss
GPC, GVC, GEC = 1.0, 0.5, 0.01
R2PI = float(np.sqrt(2 * np.pi))


def _gauss_ref(heads, acts, advs, rets, n, norm, dtype):
    """test_gpu_continuous._reference_loss (updater.py:97-98, 108-117, 124-127) in `dtype`"""
    h = heads.to(dtype).clone().requires_grad_(True)
    mu, raw, v = h[:, :n], h[:, n:2 * n], h[:, 2 * n]
    sigma = F.softplus(raw) + 1e-4
    a = advs.to(dtype)
    if norm:
        a = (a - a.mean()) / (a.std() + 1e-6)
    mse = F.mse_loss(mu, acts.to(dtype))
    ell = torch.log(torch.clamp(R2PI * sigma, min=1e-3))
    log_ps = -mse / (2 * torch.clamp(sigma ** 2, min=1e-3)) - ell
    pi_loss = GPC * -(log_ps * (a if n == 1 else a[:, None])).mean()
    val_loss = GVC * F.mse_loss(v, rets.to(dtype))
    entr = -GEC * ell.mean()
    (pi_loss + val_loss - entr).backward()
    terms = ((log_ps * (a if n == 1 else a[:, None])).detach(), ((v - rets.to(dtype)) ** 2).detach(), ell.detach())
    return torch.stack([pi_loss.detach(), val_loss.detach(), entr.detach()]), h.grad, terms


def _gauss_scale(heads, acts, advs, rets, n, norm):
    """the largest of the summed terms of a dheads element: the gradients of the quadratic part of log_ps, of its log part,
    of the entropy and of the value loss, each on its own (fp64 autograd)"""
    tot = 0.0
    for part in range(4):
        h = heads.double().clone().requires_grad_(True)
        mu, raw, v = h[:, :n], h[:, n:2 * n], h[:, 2 * n]
        sigma = F.softplus(raw) + 1e-4
        a = advs.double()
        if norm:
            a = (a - a.mean()) / (a.std() + 1e-6)
        w = a if n == 1 else a[:, None]
        ell = torch.log(torch.clamp(R2PI * sigma, min=1e-3))
        quad = -F.mse_loss(mu, acts.double()) / (2 * torch.clamp(sigma ** 2, min=1e-3))
        L = (GPC * -(quad * w).mean(), GPC * (ell * w).mean(), GEC * ell.mean(), GVC * F.mse_loss(v, rets.double()))[part]
        L.backward()
        tot = max(tot, float(h.grad.abs().max()))
    return tot


def _gauss_run(hd, ad, av, rt, asum, sums, rows, NG, n, ld_act=None):
    """the second launch on rows [lo, hi) -> (dheads, loss_sums)"""
    ops = _ops()
    lo, hi = rows
    dh = _sent(hi - lo + 2, 2 * n + 1)
    ls = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    ops.gauss_loss_fwd_bwd(hd[lo:hi, :2 * n], hd[lo:hi, 2 * n], ad[lo:hi], av[lo:hi], rt[lo:hi], asum, sums, NG, n, GPC, GVC,
                           GEC, dh[:hi - lo, :2 * n], dh[:hi - lo, 2 * n], ls)
    assert _is_sent(dh[hi - lo:])
    return dh[:hi - lo], ls.cpu()


@pytest.mark.parametrize("N,n,norm,ld_act", [(1000, 1, True, 1), (1000, 1, False, 3), (777, 2, True, 2), (1000, 32, True, 40),
                                             (150001, 2, True, 5), (150001, 3, False, 3)])
def test_gauss_loss_vs_fp64(N, n, norm, ld_act):
    """a2c_gauss_loss_sums + a2c_gauss_loss_fwd_bwd against fp64 autograd of the loss as the reference writes it; N above
    kSumsBlocks * 256 rows, n at both ends, the actions as rows of a wider buffer; twice: identical"""
    ops = _ops()
    heads = _rand_heads(N, n, 300 + N % 991 + n)
    g = _gen(N * 7 + n)
    acts = torch.randn(N, n, generator=g) * 1.3
    advs, rets = torch.randn(N, generator=g), torch.randn(N, generator=g)
    l64, g64, t64 = _gauss_ref(heads, acts, advs, rets, n, norm, torch.float64)
    l32, g32, t32 = _gauss_ref(heads, acts, advs, rets, n, norm, torch.float32)
    pi, vl, en, gref = _reference_loss(heads, heads[:, 2 * n], acts, advs, rets, n, norm, GPC, GVC, GEC)
    assert torch.allclose(gref, g64, rtol=1e-12, atol=0) and torch.allclose(torch.tensor([pi, vl, en], dtype=torch.float64), l64, rtol=1e-12)
    hd, av, rt = heads.to(DEV), advs.to(DEV), rets.to(DEV)
    awide = _sent(N, ld_act)
    awide[:, :n] = acts.to(DEV)
    ad = awide[:, :n]
    asum = _adv_sums(av) if norm else None
    outs = []
    for _ in range(2):
        sums = torch.full((6,), float("nan"), dtype=torch.float64, device=DEV)
        ops.gauss_loss_sums(hd[:, :2 * n], hd[:, 2 * n], ad, av, rt, asum, N, n, sums)
        dh, ls = _gauss_run(hd, ad, av, rt, asum, sums, (0, N), N, n)
        outs.append((sums.cpu(), dh, ls))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    sums, dh, ls = outs[0]
    got = torch.stack([GPC * -(ls[0] / N), GVC * ls[1] / N, -GEC * ls[2] / N])
    # the three values are fp64 means of fp32 per-element terms (log_ps * adv, (V - R)^2, log(sqrt(2 pi) sigma)): like the
    # discrete loss sums, every term is allowed 2 e_t + ulp, so the mean of them is too.  (Not the scalar against torch's
    # fp32 scalar: a third of the sigmas are a handful of planted values, whose few distinct roundings do not average out.)
    for i, (k, coef) in enumerate((("pi_loss", GPC), ("val_loss", GVC), ("entropy", GEC))):
        e_t = float((t32[i].double() - t64[i]).abs().max())
        ulp = float(np.spacing(np.float32(float(t64[i].abs().max()))))
        e_k = abs(float(got[i] - l64[i]))
        print(f"    gauss.{k}: |kernel - fp64| {e_k:.3e}, |torch fp32 - fp64| {abs(float(l32[i] - l64[i])):.3e}, bound {coef * (2 * e_t + ulp):.3e}")
        assert e_k <= coef * (2 * e_t + ulp), (k, float(got[i]), float(l64[i]))
    _crit("gauss.dheads", dh, g32, g64, _gauss_scale(heads, acts, advs, rets, n, norm))


@pytest.mark.parametrize("N,n1,n,norm", [(1000, 300, 1, True), (5000, 4999, 3, True), (150001, 70000, 2, False)])
def test_gauss_loss_two_shards(N, n1, n, norm):
    """two shards: each sums its rows, the six sums are added (the all-reduce), each runs the second launch with its n_local
    and the common n_global: the second launch writes share = n_local / n_global of the three values, so the two add up to
    the one-call values; with the one-call sums the gradient rows are the one-call rows bit for bit"""
    ops = _ops()
    heads = _rand_heads(N, n, 41 + n)
    g = _gen(N + n)
    acts = torch.randn(N, n, generator=g) * 1.3
    advs, rets = torch.randn(N, generator=g), torch.randn(N, generator=g)
    hd, ad, av, rt = heads.to(DEV), acts.to(DEV), advs.to(DEV), rets.to(DEV)
    asum = _adv_sums(av) if norm else None
    s_all = torch.zeros(6, dtype=torch.float64, device=DEV)
    ops.gauss_loss_sums(hd[:, :2 * n], hd[:, 2 * n], ad, av, rt, asum, N, n, s_all)
    dh_all, ls_all = _gauss_run(hd, ad, av, rt, asum, s_all, (0, N), N, n)
    shard_sums = []
    for lo, hi in ((0, n1), (n1, N)):
        s = torch.full((6,), float("nan"), dtype=torch.float64, device=DEV)
        ops.gauss_loss_sums(hd[lo:hi, :2 * n], hd[lo:hi, 2 * n], ad[lo:hi], av[lo:hi], rt[lo:hi], asum, N, n, s)
        shard_sums.append(s)
    added = shard_sums[0] + shard_sums[1]
    # the same fp32 row sums in another fp64 order: N * 2^-53 (1e-12 for short batches) of the sum of their magnitudes, which
    # is below 4000 n per row (|w| < 8 over 2 c >= 2e-3; |l| < 7, d^2 < 400)
    assert float((added - s_all).abs().max()) <= max(1e-12, N * 2.0 ** -53) * (N * n * 4000.0)
    ls_sum = torch.zeros(3, dtype=torch.float64)
    for lo, hi in ((0, n1), (n1, N)):
        dh, ls = _gauss_run(hd, ad, av, rt, asum, s_all, (lo, hi), N, n)
        assert torch.equal(dh, dh_all[lo:hi]), "a shard's gradient rows differ from the one-call rows"
        share = (hi - lo) / N
        assert torch.allclose(ls, ls_all * share, rtol=4e-16, atol=0), (ls, ls_all, share)
        ls_sum += ls
        dh2, ls2 = _gauss_run(hd, ad, av, rt, asum, added, (lo, hi), N, n)       # the all-reduced sums: one fp32 ulp at most
        assert float((dh2 - dh).abs().max()) <= float(np.spacing(np.float32(float(dh.abs().max()))))
    assert torch.allclose(ls_sum, ls_all, rtol=1e-15, atol=0)
    z = torch.full((6,), 3.0, dtype=torch.float64, device=DEV)
    ops.gauss_loss_sums(hd[:0, :2 * n], hd[:0, 2 * n], ad[:0], av[:0], rt[:0], asum, N, n, z)       # n_local = 0
    assert bool((z == 0).all())


# ====================================================================================================== GRU elementwise
GRU_SHAPES = [(1, 1), (3, 7), (37, 64), (256, 256), (4099, 257)]      # the last: > 2048 * 256 elements (grid-stride)


def _sig(x):
    return torch.sigmoid(x)


def _gru_inputs(B, h, seed):
    """Bp = enough rows for POOL * 8 elements; a planted tenth of the z / r pre-activations beyond +-90"""
    Bp = max(B, (8 * POOL + h - 1) // h)
    gx, gh = _u((Bp, 3 * h), seed, -2, 2), _u((Bp, 2 * h), seed + 1, -2, 2)
    sat = torch.rand(Bp, 2 * h, generator=_gen(seed + 2)) < 0.1
    sgn = torch.where(torch.rand(Bp, 2 * h, generator=_gen(seed + 3)) < 0.5, -1.0, 1.0)
    gx[:, :2 * h][sat] = (sgn * _u((Bp, 2 * h), seed + 4, 95, 120))[sat]
    b, hin, rhu = _u((3 * h,), seed + 5) * 0.1, _u((Bp, h), seed + 6), _u((Bp, h), seed + 7, -2, 2)
    return gx, gh, b, hin, rhu, sat


def _gru_fwd_ref(gx, gh, b, hin, rhu, dtype):
    """models.py:465-476 with the matrix products given"""
    h = hin.shape[1]
    gx, gh, b, hin, rhu = (t.to(dtype) for t in (gx, gh, b, hin, rhu))
    z = _sig((gx[:, :h] + gh[:, :h]) + b[:h])
    r = _sig((gx[:, h:2 * h] + gh[:, h:]) + b[h:2 * h])
    c = torch.tanh((gx[:, 2 * h:] + rhu) + b[2 * h:])
    return dict(z=z, r=r, rh=r * hin, c=c, hn=z * hin + (1 - z) * c)


@pytest.mark.parametrize("B,h", GRU_SHAPES)
def test_gru_gates_and_out_vs_fp64(B, h):
    """a2c_gru_gates / a2c_gru_out: every output against fp64; saturated gates are exactly 0 or 1 and nothing is NaN;
    c = NULL; h_new written over h"""
    ops = _ops()
    gx, gh, b, hin, rhu, sat = _gru_inputs(B, h, 2000 + B + h)
    r64, r32 = _gru_fwd_ref(gx, gh, b, hin, rhu, torch.float64), _gru_fwd_ref(gx, gh, b, hin, rhu, torch.float32)
    dev = lambda t: t[:B].to(DEV).contiguous()
    gxd, ghd, bd, hd, rhud = dev(gx), dev(gh), b.to(DEV), dev(hin), dev(rhu)
    z, r, rh, c, hn = (_sent(B + 1, h) for _ in range(5))
    ops.gru_gates(gxd, ghd, bd, hd, z[:B], r[:B], rh[:B])
    ops.gru_out(gxd, rhud, bd, hd, z[:B].contiguous(), c[:B], hn[:B])
    for t in (z, r, rh, c, hn):
        assert _is_sent(t[B:]) and bool(torch.isfinite(t).all())
    zr = torch.cat([z[:B], r[:B]], 1).cpu()
    s = sat[:B]
    pre = gx[:B, :2 * h].double() + gh[:B].double() + b[:2 * h].double()
    assert bool((pre[s].abs() > 90).all())
    assert bool(((zr[s] == 0) | (zr[s] == 1)).all()) and torch.equal(zr[s], (pre[s] > 0).float())
    if B * h >= 64:
        assert bool(s.any())
    _crit("gru_gates.z", z[:B], r32["z"], r64["z"])
    _crit("gru_gates.r", r[:B], r32["r"], r64["r"])
    _crit("gru_gates.rh", rh[:B], r32["rh"], r64["rh"])
    # the out kernel read the KERNEL's z: the reference of h_new with that z would hide nothing, but the criterion is about
    # the formula, so z's own error (<= its bound above) stays inside e_k
    _crit("gru_out.c", c[:B], r32["c"], r64["c"])
    hn_scale = max(float((r64["z"] * hin.double()).abs().max()), float(((1 - r64["z"]) * r64["c"]).abs().max()))
    _crit("gru_out.h_new", hn[:B], r32["hn"], r64["hn"], hn_scale)
    # c = NULL and h_new over h: the same h_new bit for bit
    h_io = hd.clone()
    ops.gru_out(gxd, rhud, bd, h_io, z[:B].contiguous(), None, h_io)
    assert torch.equal(h_io, hn[:B])


def _gru_bwd_ref(dhn, carry, done, hin, z, c, r, d_rh, dh0, dtype):
    """updater.py:139-169 differentiated through models.py:465-476, the elementwise stages; z, r, c are the saved fp32
    activations"""
    dhn, carry, done, hin, z, c, r, d_rh, dh0 = (t.to(dtype) for t in (dhn, carry, done, hin, z, c, r, d_rh, dh0))
    out = {}
    for name, g in (("", dhn), ("_carry", dhn + carry * (1 - done)[:, None])):
        out["dc_pre" + name] = g * (1 - z) * (1 - c * c)
        out["dz" + name] = g * (hin - c)
        out["dh" + name] = g * z
        out["g" + name] = g
    out["dz_pre"] = out["dz"] * z * (1 - z)
    out["dr_pre"] = d_rh * hin * r * (1 - r)
    out["dh_acc"] = dh0 + d_rh * r
    return out


@pytest.mark.parametrize("B,h", GRU_SHAPES)
def test_gru_backward_elementwise_vs_fp64(B, h):
    """a2c_gru_out_bwd, a2c_gru_out_bwd_carry (carry IS dh; done read at a stride, beside columns that say the opposite)
    and a2c_gru_gates_bwd accumulating into a dh that is not zero"""
    ops = _ops()
    gx, gh, b, hin, rhu, _ = _gru_inputs(B, h, 2100 + B + h)
    Bp = hin.shape[0]
    f = _gru_fwd_ref(gx, gh, b, hin, rhu, torch.float32)
    z, r, c = f["z"], f["r"], f["c"]
    dhn, carry, d_rh, dh0 = (_u((Bp, h), 2200 + i) for i in range(4))
    # done of row b at dones[b, 1]; the rows cycle through all 0, all 1, and the two mixed patterns
    pats = torch.tensor([[0., 0, 0], [1, 1, 1], [1, 0, 1], [0, 1, 0]])
    dones = pats[torch.arange(Bp) % 4]
    if B >= 4:
        for p in pats:
            assert bool((dones[:B] == p).all(1).any())
    done = dones[:, 1]
    r64 = _gru_bwd_ref(dhn, carry, done, hin, z, c, r, d_rh, dh0, torch.float64)
    r32 = _gru_bwd_ref(dhn, carry, done, hin, z, c, r, d_rh, dh0, torch.float32)
    dev = lambda t: t[:B].to(DEV).contiguous()
    dhnd, hd, zd, cd, rd, drhd = dev(dhn), dev(hin), dev(z), dev(c), dev(r), dev(d_rh)
    dd = dev(dones)
    gmax = float(r64["g_carry"].abs().max())
    hc = max(float(hin.abs().max()), float(c.abs().max()))
    for name, use_carry in (("gru_out_bwd", False), ("gru_out_bwd_carry", True)):
        dcp, dz = _sent(B + 1, h), _sent(B + 1, h)
        dh = _sent(B + 1, h)
        sfx = "_carry" if use_carry else ""
        if use_carry:
            dh[:B] = dev(carry)
            ops.gru_out_bwd_carry(dhnd, dh[:B], dd.data_ptr() + 4, 3, hd, zd, cd, dcp[:B], dz[:B], dh[:B])
        else:
            ops.gru_out_bwd(dhnd, hd, zd, cd, dcp[:B], dz[:B], dh[:B])
        assert _is_sent(dcp[B:]) and _is_sent(dz[B:]) and _is_sent(dh[B:])
        # dc_pre = g (1 - z) (1 - c^2): the two differences are of terms of size 1; dz = g h - g c
        _crit(f"{name}.dc_pre", dcp[:B], r32["dc_pre" + sfx], r64["dc_pre" + sfx], gmax)
        _crit(f"{name}.dz", dz[:B], r32["dz" + sfx], r64["dz" + sfx], gmax * hc)
        _crit(f"{name}.dh", dh[:B], r32["dh" + sfx], r64["dh" + sfx], gmax)
    dzp, drp, dh = _sent(B + 1, h), _sent(B + 1, h), _sent(B + 1, h)
    dh[:B] = dev(dh0)
    dz_in = dev(r32["dz"])
    ops.gru_gates_bwd(drhd, dz_in, hd, zd, rd, dzp[:B], drp[:B], dh[:B])
    assert _is_sent(dzp[B:]) and _is_sent(drp[B:]) and _is_sent(dh[B:])
    dzp64 = r32["dz"].double() * z.double() * (1 - z.double())          # from the fp32 dz the kernel was given
    dzp32 = r32["dz"] * z * (1 - z)
    # dz z (1 - z), d_rh h r (1 - r): the difference is of terms of size 1, times a product of size max|dz z|, max|d_rh h r|
    _crit("gru_gates_bwd.dz_pre", dzp[:B], dzp32, dzp64, float(r32["dz"].abs().max()))
    _crit("gru_gates_bwd.dr_pre", drp[:B], r32["dr_pre"], r64["dr_pre"], float((d_rh * hin).abs().max()))
    _crit("gru_gates_bwd.dh", dh[:B], r32["dh_acc"], r64["dh_acc"], max(float(dh0.abs().max()), float(d_rh.abs().max())))


# ====================================================================================================== GRU cell
CELL_HD = [32, 64, 96, 128, 160, 512]
CELL_XS = [8, 24, 72, 264]
CELL_B = [1, 31, 32, 33, 257]


def wave_kinds(K, NWK, with_head):
    """what each of the NWK waves of a product does with its K range (rnn.hip: kq = ceil(K / 8 / NWK) * 8): 'empty', or
    with the x / h side's two-group loop 'head' (one 8-group only), 'head+loop', 'loop'; the backward's k-contiguous loop
    has no head: 'loop'"""
    kq = ((K // 8 + NWK - 1) // NWK) * 8
    kinds = []
    for w in range(NWK):
        kbeg = min(K, w * kq)
        kend = min(K, kbeg + kq)
        n = kend - kbeg
        if n == 0:
            kinds.append("empty")
        elif not with_head:
            kinds.append("loop")
        else:
            head = (n & 15) != 0
            loops = (n - (8 if head else 0)) // 16
            kinds.append("head" if head and not loops else "head+loop" if head else "loop")
    return kinds


def five_launches_comparable(B, hd, xs=None):
    """a2c_gemm_f32 runs every product of the five launches on the four-wave small-product kernel the cell kernels
    reproduce (its dispatch: K % 8 == 0, 32 <= K < 1024, fewer than 64 tiles of 128 x 128 and at least 16 of 32 x 32, or 4
    when M <= 32); elsewhere (one row, xs = 8 or 24, few tiles) the five launches are another kernel and another sum"""
    def small(M, N, K):
        t128, t32 = ((M + 127) // 128) * ((N + 127) // 128), ((M + 31) // 32) * ((N + 31) // 32)
        return M > 8 and K % 8 == 0 and 32 <= K < 1024 and t128 < 64 and (t32 >= 16 or (M <= 32 and t32 >= 4)) and t32 <= 4096
    prods = [(B, hd, hd)] if xs is None else [(B, 3 * hd, xs), (B, 2 * hd, hd), (B, hd, hd)]
    return all(small(*p) for p in prods)


def test_gru_cell_case_list_reaches_every_kind_of_wave():
    """on the CPU, before anything is sent to the GPU: over the (K, NWK) of the forward cases every kind of wave occurs --
    empty, head only, head plus loop, loop only -- for both splits, and for the backward idle and working waves"""
    for NWK in (4, 8):
        seen = set()
        for K in CELL_XS + CELL_HD:
            seen.update(wave_kinds(K, NWK, True))
        assert seen == {"empty", "head", "head+loop", "loop"}, (NWK, seen)
        seen_b = set()
        for K in CELL_HD:
            seen_b.update(wave_kinds(K, NWK, False))
        # (hd is a multiple of 32: four 8-groups at least, so only the eight-way split can leave a wave of the backward idle)
        assert seen_b == ({"empty", "loop"} if NWK == 8 else {"loop"}), (NWK, seen_b)
    assert sum(five_launches_comparable(B, hd, xs) for B in CELL_B for hd in CELL_HD for xs in CELL_XS) >= 20
    assert sum(five_launches_comparable(B, hd) for B in CELL_B for hd in CELL_HD) >= 10
    assert wave_kinds(32, 8, True) == ["head"] * 4 + ["empty"] * 4
    assert wave_kinds(8, 8, True) == ["head"] + ["empty"] * 7
    assert wave_kinds(72, 4, True) == ["head+loop"] * 3 + ["empty"]
    assert wave_kinds(264, 8, True) == ["head+loop"] * 6 + ["head+loop", "empty"]



def _cell_weights(xs, hd, seed):
    Wx, Wh = _u((3, xs, hd), seed) / xs ** 0.5, _u((3, hd, hd), seed + 1) / hd ** 0.5
    return Wx, Wh, _u((3 * hd,), seed + 2) * 0.1


def _cell_fwd_ref(x, h, Wx, Wh, b, dtype):
    hd = h.shape[1]
    x, h, Wx, Wh, b = (t.to(dtype) for t in (x, h, Wx, Wh, b))
    z = _sig(x.mm(Wx[0]) + h.mm(Wh[0]) + b[:hd])
    r = _sig(x.mm(Wx[1]) + h.mm(Wh[1]) + b[hd:2 * hd])
    gx2 = x.mm(Wx[2])
    c = torch.tanh(gx2 + (r * h).mm(Wh[2]) + b[2 * hd:])
    return dict(z=z, r=r, rh=r * h, c=c, hn=z * h + (1 - z) * c, gx2=gx2)


@pytest.mark.parametrize("k4", [True, False])
@pytest.mark.parametrize("xs", CELL_XS)
@pytest.mark.parametrize("hd", CELL_HD)
def test_gru_cell_fwd_vs_fp64(hd, xs, k4, monkeypatch):
    """a2c_gru_cell_fwd with both K splits, every output against fp64 on its own; x as rows of a wider buffer; rows past B of
    the last 32-row tile untouched; with A2C_GRU_K4=1 bit for bit the five launches it replaces"""
    ops = _ops()
    monkeypatch.setenv("A2C_GRU_K4", "1" if k4 else "0")
    Bp = max(CELL_B)
    x, h0 = _u((Bp, xs), 3000 + hd + xs, 0, 1), _u((Bp, hd), 3001 + hd + xs)
    Wx, Wh, b = _cell_weights(xs, hd, 3002 + hd + xs)
    r64, r32 = _cell_fwd_ref(x, h0, Wx, Wh, b, torch.float64), _cell_fwd_ref(x, h0, Wx, Wh, b, torch.float32)
    xw = _sent(Bp, xs + 12)
    xw[:, :xs] = x.to(DEV)
    xd = xw[:, :xs]
    hdv, bd = h0.to(DEV), b.to(DEV)
    Wxd, Whd = Wx.to(DEV), Wh.to(DEV)
    WxC = torch.cat([Wxd[g] for g in range(3)], 1).contiguous()
    WhC = torch.cat([Whd[g] for g in range(2)], 1).contiguous()
    # the largest product summed into a pre-activation, and what it does to each output (sigmoid' <= 1/4, tanh' <= 1)
    tx = float(x.abs().max() * Wx.abs().max())
    th = float(h0.abs().max() * Wh.abs().max())
    pre = max(tx, th, float(b.abs().max()))
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    for B in CELL_B:
        gx, z, r, rh, c, hn = nan(B + 32, 3 * hd), nan(B + 32, hd), nan(B + 32, hd), nan(B + 32, hd), nan(B + 32, hd), nan(B + 32, hd)
        ops.gru_cell_fwd(xd[:B], hdv[:B], WxC, WhC, Whd[2], bd, gx, z, r, rh, c, hn)
        for name, t in (("gx", gx), ("z", z), ("r", r), ("rh", rh), ("c", c), ("hn", hn)):
            assert bool(torch.isnan(t[B:]).all()), f"{name}: a row past B was written (B = {B})"
        assert bool(torch.isnan(gx[:B, :2 * hd]).all())
        tag = "gru_cell_fwd" + ("_k4" if k4 else "")
        _crit(f"{tag}.gx2 B={B}", gx[:B, 2 * hd:], r32["gx2"], r64["gx2"], tx)
        for k, t, amp in (("z", z, 0.25), ("r", r, 0.25), ("rh", rh, 0.25), ("c", c, 1.0), ("hn", hn, 1.0)):
            _crit(f"{tag}.{k} B={B}", t[:B], r32[k], r64[k], max(amp * pre, float(r64[k].abs().max())))
        if k4 and five_launches_comparable(B, hd, xs):      # the five launches, bit for bit
            gx5, gh5, z5, r5, rh5, rhu5, c5, hn5 = nan(B, 3 * hd), nan(B, 2 * hd), nan(B, hd), nan(B, hd), nan(B, hd), nan(B, hd), nan(B, hd), nan(B, hd)
            ops.gemm(0, 0, B, 3 * hd, xs, xd.data_ptr(), xd.stride(0), WxC.data_ptr(), 3 * hd, gx5.data_ptr(), 3 * hd)
            ops.gemm(0, 0, B, 2 * hd, hd, hdv.data_ptr(), hd, WhC.data_ptr(), 2 * hd, gh5.data_ptr(), 2 * hd)
            ops.gru_gates(gx5, gh5, bd, hdv[:B], z5, r5, rh5)
            ops.gemm(0, 0, B, hd, hd, rh5.data_ptr(), hd, Whd[2].data_ptr(), hd, rhu5.data_ptr(), hd)
            ops.gru_out(gx5, rhu5, bd, hdv[:B], z5, c5, hn5)
            for name, a, bb in (("z", z, z5), ("r", r, r5), ("rh", rh, rh5), ("c", c, c5), ("hn", hn, hn5),
                                ("gx2", gx[:, 2 * hd:], gx5[:, 2 * hd:])):
                assert torch.equal(a[:B], bb), f"{name}: A2C_GRU_K4=1 is not the five launches bit for bit (B = {B})"
    assert _is_sent(xw[:, xs:])


def _cell_bwd_ref(dhn, carry, done, h, z, r, c, Wh, dtype):
    dhn, h, z, r, c, Wh = (t.to(dtype) for t in (dhn, h, z, r, c, Wh))
    g = dhn if carry is None else dhn + carry.to(dtype) * (1 - done.to(dtype))[:, None]
    dcp = g * (1 - z) * (1 - c * c)
    dz = g * (h - c)
    drh = dcp.mm(Wh[2].t())
    dzp = dz * z * (1 - z)
    drp = drh * h * r * (1 - r)
    dh = g * z + drh * r + dzp.mm(Wh[0].t()) + drp.mm(Wh[1].t())
    return dict(dc_pre=dcp, dz=dz, dz_pre=dzp, dr_pre=drp, dh=dh, g=g, drh=drh)


@pytest.mark.parametrize("k4", [True, False])
@pytest.mark.parametrize("hd", CELL_HD)
def test_gru_cell_bwd_vs_fp64(hd, k4, monkeypatch):
    """a2c_gru_cell_bwd with both K splits against fp64 for all five outputs, with and without the carry (done read at a
    stride); rows past B untouched; with A2C_GRU_K4=1 bit for bit the five launches"""
    ops = _ops()
    monkeypatch.setenv("A2C_GRU_K4", "1" if k4 else "0")
    Bp = max(CELL_B)
    x, h0 = _u((Bp, hd), 3100 + hd, 0, 1), _u((Bp, hd), 3101 + hd)
    Wx, Wh, b = _cell_weights(hd, hd, 3102 + hd)
    f = _cell_fwd_ref(x, h0, Wx, Wh, b, torch.float32)
    z, r, c = f["z"], f["r"], f["c"]
    dhn, carry = _u((Bp, hd), 3103 + hd), _u((Bp, hd), 3104 + hd)
    dones = (torch.rand(Bp, 3, generator=_gen(3105 + hd)) < 0.3).float()
    dones[0, 1], dones[1 % Bp, 1] = 1.0, 0.0
    hdv, zd, rd, cd, Whd, dhnd, cyd, dd = (t.to(DEV).contiguous() for t in (h0, z, r, c, Wh, dhn, carry, dones))
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    for i, B in enumerate(CELL_B):
        with_carry = (i + hd // 32) % 2 == 0 or B == 257
        cy = carry if with_carry else None
        r64 = _cell_bwd_ref(dhn, cy, dones[:, 1], h0, z, r, c, Wh, torch.float64)
        r32 = _cell_bwd_ref(dhn, cy, dones[:, 1], h0, z, r, c, Wh, torch.float32)
        outs = [nan(B + 32, hd) for _ in range(5)]
        v = [t[:B] for t in outs]
        ops.gru_cell_bwd(dhnd[:B], cyd[:B] if with_carry else None, dd.data_ptr() + 4 if with_carry else 0, 3, hdv[:B], zd[:B],
                         rd[:B], cd[:B], Whd, *v)
        for t in outs:
            assert bool(torch.isnan(t[B:]).all()), f"a row past B was written (B = {B})"
        gmax = float(r64["g"].abs().max())
        t_rh = float(r64["dc_pre"].abs().max() * Wh[2].abs().max())          # largest product summed into d_rh
        t_dh = max(gmax, float(r64["drh"].abs().max()), float(r64["dz_pre"].abs().max() * Wh[0].abs().max()),
                   float(r64["dr_pre"].abs().max() * Wh[1].abs().max()))
        tag = "gru_cell_bwd" + ("_k4" if k4 else "")
        _crit(f"{tag}.dc_pre B={B}", v[0], r32["dc_pre"], r64["dc_pre"], gmax)
        _crit(f"{tag}.dz B={B}", v[1], r32["dz"], r64["dz"], gmax)
        _crit(f"{tag}.dz_pre B={B}", v[2], r32["dz_pre"], r64["dz_pre"], float(r64["dz"].abs().max()))
        _crit(f"{tag}.dr_pre B={B}", v[3], r32["dr_pre"], r64["dr_pre"], t_rh)
        _crit(f"{tag}.dh B={B}", v[4], r32["dh"], r64["dh"], t_dh)
        if k4 and five_launches_comparable(B, hd):
            dcp1, dz1, drh1, dzp1, drp1, dh1 = (nan(B, hd) for _ in range(6))
            if with_carry:
                ops.gru_out_bwd_carry(dhnd[:B], cyd[:B], dd.data_ptr() + 4, 3, hdv[:B], zd[:B], cd[:B], dcp1, dz1, dh1)
            else:
                ops.gru_out_bwd(dhnd[:B], hdv[:B], zd[:B], cd[:B], dcp1, dz1, dh1)
            ops.gemm(0, 1, B, hd, hd, dcp1.data_ptr(), hd, Whd[2].data_ptr(), hd, drh1.data_ptr(), hd)
            ops.gru_gates_bwd(drh1, dz1, hdv[:B], zd[:B], rd[:B], dzp1, drp1, dh1)
            ops.gemm(0, 1, B, hd, hd, dzp1.data_ptr(), hd, Whd[0].data_ptr(), hd, dh1.data_ptr(), hd, accumulate=True)
            ops.gemm(0, 1, B, hd, hd, drp1.data_ptr(), hd, Whd[1].data_ptr(), hd, dh1.data_ptr(), hd, accumulate=True)
            for name, a, bb in zip(("dc_pre", "dz", "dz_pre", "dr_pre", "dh"), v, (dcp1, dz1, dzp1, drp1, dh1)):
                assert torch.equal(a, bb), f"{name}: A2C_GRU_K4=1 is not the five launches bit for bit (B = {B})"


# ====================================================================================================== LayerNorm
LN_N = [1, 2, 63, 64, 65, 200, 256, 1000]
LN_ROWS = [1, 3, 4, 5, 53, 8195]          # 8195 > 4 * 2048: rows revisited by grid-stride


def _ln_ref(x, w, b, dy, dx0, dtype):
    """torch.nn.LayerNorm (models.py:392, 510) forward and backward, with the saved mean and rstd"""
    x, w, b, dy, dx0 = (t.to(dtype) for t in (x, w, b, dy, dx0))
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    n = x.shape[1]
    y, mean, rstd = torch.native_layer_norm(xr, (n,), wr, b, 1e-5)
    y.backward(dy)
    xh = (x - mean) * rstd
    return dict(y=y.detach(), mean=mean.detach().flatten(), rstd=rstd.detach().flatten(), dx=xr.grad, dx_acc=dx0 + xr.grad,
                dw_rows=dy * xh, dw=wr.grad, xh=xh)


@pytest.mark.parametrize("offset", [0.0, 1e3])
@pytest.mark.parametrize("n", LN_N)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_layernorm_vs_fp64(rows, n, offset):
    """a2c_layernorm_fwd / _bwd: y, mean, rstd, dx (accum 0 and 1), dw_rows per row and their column sum through a2c_colsum;
    unit spread around 0 and around 1e3 (where a one-pass variance is lost), every fifth row constant"""
    ops = _ops()
    Rp = max(rows, (4 * POOL + n - 1) // n)
    seed = 4000 + rows + n
    x = _nrm((Rp, n), seed) + offset
    x[2::5] = 0.5 + offset
    w, b = 1 + 0.1 * _u((n,), seed + 1), 0.1 * _u((n,), seed + 2)
    dy, dx0 = _u((Rp, n), seed + 3), _u((Rp, n), seed + 4)
    if rows >= 3:
        assert bool((x[:rows] == x[:rows, :1]).all(1).any())
    r64, r32 = _ln_ref(x, w, b, dy, dx0, torch.float64), _ln_ref(x, w, b, dy, dx0, torch.float32)
    dev = lambda t: t[:rows].to(DEV).contiguous()
    xd, wd, bd, dyd = dev(x), w.to(DEV), b.to(DEV), dev(dy)
    y, mean, rstd = _sent(rows + 1, n), _sent(rows + 1), _sent(rows + 1)
    ops.layernorm_fwd(xd, wd, bd, y[:rows], mean[:rows], rstd[:rows])
    assert _is_sent(y[rows:]) and _is_sent(mean[rows:]) and _is_sent(rstd[rows:])
    xmax = float(x.abs().max())
    _crit("layernorm_fwd.mean", mean[:rows], r32["mean"], r64["mean"], xmax)
    # rstd = 1 / sqrt(var + eps): the relative error of var is that of the largest (x - mean)^2 in it
    _crit("layernorm_fwd.rstd", rstd[:rows], r32["rstd"], r64["rstd"])
    ymax = max(float((r64["xh"] * w.double()).abs().max()), float(b.abs().max()))
    _crit("layernorm_fwd.y", y[:rows], r32["y"], r64["y"], ymax)
    # dx = rstd (dy w - s1 - xhat s2): the largest of the three terms
    g = dy.double() * w.double()
    s1 = g.mean(1, keepdim=True)
    s2 = (g * r64["xh"]).mean(1, keepdim=True)
    rs = r64["rstd"][:, None]
    t_dx = max(float((rs * g).abs().max()), float((rs * s1).abs().max()), float((rs * r64["xh"] * s2).abs().max()))
    for accum in (0, 1):
        dx, dwr = _sent(rows + 1, n), _sent(rows + 1, n)
        if accum:
            dx[:rows] = dev(dx0)
        ops.layernorm_bwd(dyd, xd, wd, mean[:rows].contiguous(), rstd[:rows].contiguous(), dx[:rows], dwr[:rows], accumulate=bool(accum))
        assert _is_sent(dx[rows:]) and _is_sent(dwr[rows:])
        if accum:
            _crit("layernorm_bwd.dx accum", dx[:rows], r32["dx_acc"], r64["dx_acc"], max(t_dx, float(dx0.abs().max())))
        else:
            _crit("layernorm_bwd.dx", dx[:rows], r32["dx"], r64["dx"], t_dx)
        _crit("layernorm_bwd.dw_rows", dwr[:rows], r32["dw_rows"], r64["dw_rows"])
    ws = torch.empty(max(1, ops.colsum_ws_bytes(n) // 4), device=DEV)
    dw = _sent(n + 1)
    ops.colsum(dwr.data_ptr(), n, rows, n, dw[:n], ws)
    assert _is_sent(dw[n:])
    # the column sum of the rows the backward kernel wrote (each checked above): fp64 and the running fp32 sum of those rows
    rows_k = dwr[:rows].cpu()
    _crit("layernorm_bwd.dw colsum", dw[:n], _running_sum(rows_k), rows_k.double().sum(0), float(rows_k.abs().max()))


# ====================================================================================================== moments / normalize / add
MOM_N = [1, 2, 257, 262144, 262145, 3000001]       # 262 144 = 1024 * 256: the last size of one pass


def _fsums(x):
    v = x.double().tolist()
    return math.fsum(v), math.fsum(t * t for t in v)


@pytest.mark.parametrize("kind", ["spread", "constant", "offset"])
@pytest.mark.parametrize("n", MOM_N)
def test_moments_normalize_add_vs_fp64(n, kind):
    """a2c_moments: fp64 sums of the fp32 values and of their (exact) fp64 squares, against math.fsum to 1e-12 -- n * 2^-53
    at the largest n is 3.3e-10 of the sum of magnitudes in the worst case and 2^-53 sqrt(n) = 2e-13 in the mean;
    a2c_normalize (updater.py:97-98) against fp64; a2c_add is one rounding: exact"""
    ops = _ops()
    x = {"spread": lambda: _u((n,), 5000 + n, -3, 5), "constant": lambda: torch.full((n,), 0.75),
         "offset": lambda: _nrm((n,), 5001 + n) + 1e4}[kind]()
    xb = _sent(n + 3)
    xb[:n] = x.to(DEV)
    xd = xb[:n]
    sums = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    ops.moments(xd, sums)
    s1, s2 = _fsums(x)
    got = sums.cpu().tolist()
    print(f"    moments n={n} {kind}: rel err {abs(got[0] - s1) / max(abs(s1), 1e-300):.2e} {abs(got[1] - s2) / s2:.2e}")
    a1 = math.fsum(abs(t) for t in x.double().tolist())
    assert abs(got[0] - s1) <= 1e-12 * a1 and abs(got[1] - s2) <= 1e-12 * s2
    sums2 = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    ops.moments(xd, sums2)
    assert torch.equal(sums, sums2)
    yb = _sent(n + 3)
    if n == 1:
        _raises(ERR_ARG, ops.normalize, xd, yb[:n], sums, 1, 1e-6)
        assert _is_sent(yb)
    else:
        ops.normalize(xd, yb[:n], sums, n, 1e-6)
        assert _is_sent(yb[n:])
        ref = lambda t: (t - t.mean()) / (t.std() + 1e-6)
        r64, r32 = ref(x.double()), ref(x)
        if kind == "constant":
            assert float(yb[:n].abs().max()) == 0.0 and float(r64.abs().max()) == 0.0
        else:
            # (x - mean) / den: the difference is of terms of size max|x|, then divided by den
            den = float(x.double().std() + 1e-6)
            _crit(f"normalize {kind}", yb[:n], r32, r64, float(x.abs().max()) / den)
    zb = _sent(n + 3)
    other = _u((n,), 5002 + n, -7, 7)
    ops.add(xd, other.to(DEV), zb[:n])
    assert torch.equal(zb[:n].cpu(), x + other) and _is_sent(zb[n:])


@pytest.mark.parametrize("n,n1", [(5000, 1234), (262145, 262144), (2, 1)])
def test_moments_of_two_shards_normalise_like_one(n, n1):
    """n_global > n: each shard's sums added (the all-reduce), each shard normalised with the global count"""
    ops = _ops()
    x = _u((n,), 5100 + n, -3, 5)
    xd = x.to(DEV)
    parts = []
    for lo, hi in ((0, n1), (n1, n)):
        s = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
        ops.moments(xd[lo:hi].contiguous(), s)
        parts.append(s)
    tot = parts[0] + parts[1]
    s1, s2 = _fsums(x)
    assert abs(float(tot[0]) - s1) <= 1e-12 * float(x.double().abs().sum()) and abs(float(tot[1]) - s2) <= 1e-12 * s2
    y = _sent(n)
    for lo, hi in ((0, n1), (n1, n)):
        ops.normalize(xd[lo:hi].contiguous(), y[lo:hi], tot, n, 1e-6)
    ref = lambda t: (t - t.mean()) / (t.std() + 1e-6)
    if n >= 100:
        _crit("normalize shards", y, ref(x), ref(x.double()), float(x.abs().max()) / float(x.double().std() + 1e-6))
    else:
        assert torch.allclose(y.cpu().double(), ref(x.double()), rtol=0, atol=4 * float(np.spacing(np.float32(5 / x.double().std()))))


def test_moments_of_nothing_are_zero():
    ops = _ops()
    s = torch.full((2,), 5.0, dtype=torch.float64, device=DEV)
    ops.moments(torch.empty(0, device=DEV), s)
    assert bool((s == 0).all())


# ====================================================================================================== samplers
SAMPLE_A = [1, 2, 3, 6, 18, 32]
SAMPLE_B = [1, 777, 600001]          # 600 001 > 2048 * 256: rows revisited by grid-stride
MARGIN = 1e-5                        # an fp32 running sum of <= 32 probabilities is within 32 * 2^-24 = 1.9e-6 of fp64's


def draw_uniforms_clear_of_the_cumsum(p64, seed):
    """u in [0, 1) such that no row has |cs_a - u| < MARGIN for any a, cs the fp64 running sum: offending rows are drawn
    again from the next seed until none is left"""
    B = p64.shape[0]
    cs = torch.cumsum(p64, -1)
    u = torch.rand(B, generator=_gen(seed))
    for k in range(1, 200):
        bad = ((cs - u.double()[:, None]).abs() < MARGIN).any(1).nonzero().flatten()
        if bad.numel() == 0:
            break
        u[bad] = torch.rand(bad.numel(), generator=_gen(seed + 7919 * k))
    assert not bool(((cs - u.double()[:, None]).abs() < MARGIN).any()), "a uniform within the margin of a cumulative sum"
    return u


@pytest.mark.parametrize("A", SAMPLE_A)
def test_uniform_draw_keeps_its_margin_on_the_cpu(A):
    for B in SAMPLE_B[:2] + [20001]:
        p64 = F.softmax(_u((B, A), 6000 + A + B, -4, 4).double(), -1)
        u = draw_uniforms_clear_of_the_cumsum(p64, 6100 + A)
        cs = torch.cumsum(p64, -1)
        assert float((cs - u.double()[:, None]).abs().min()) >= MARGIN and float(u.max()) < 1 - MARGIN and float(u.min()) >= 0



@pytest.mark.parametrize("B", SAMPLE_B)
@pytest.mark.parametrize("A", SAMPLE_A)
def test_samplers_vs_oracle_with_zero_mismatches(A, B):
    """a2c_softmax_sample and a2c_sample_probs (utils.py:45-60) against the oracle's sample_action on fp32 softmax, on
    uniforms kept MARGIN clear of every fp64 cumulative sum: the actions are equal on every row; the probabilities against
    fp64; the strided actions keep their neighbours"""
    ops = _ops()
    wide = _u((B, A + 2), 6000 + A + B, -4, 4)
    logits = wide[:, 1:A + 1]
    p64, p32 = F.softmax(logits.double(), -1), F.softmax(logits, -1)
    u = draw_uniforms_clear_of_the_cumsum(p64, 6100 + A)
    want = O.sample_action(p32, u)
    assert int((want < 0).sum()) == 0
    want64 = (torch.cumsum(p64, -1) < u.double()[:, None]).sum(1)
    assert torch.equal(want.long(), want64), "fp32 and fp64 inverse CDF disagree despite the margin"
    ld, ud = wide.to(DEV)[:, 1:A + 1], u.to(DEV)
    acts = torch.full((B + 1, 3), -7, dtype=torch.int64, device=DEV)
    probs = _sent(B + 1, A)
    ops.softmax_sample(ld, ud, acts.data_ptr() + 8, 3, B, A, probs=probs[:B])
    assert torch.equal(acts[:B, 1].cpu(), want.long()), f"{int((acts[:B, 1].cpu() != want.long()).sum())} sampled actions differ"
    assert bool((acts[:, 0] == -7).all()) and bool((acts[:, 2] == -7).all()) and int(acts[B, 1]) == -7 and _is_sent(probs[B:])
    _crit("softmax_sample.probs", probs[:B], p32, p64)
    acts2 = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    ops.softmax_sample(ld, ud, acts2.data_ptr(), 1, B, A, probs=None)
    assert torch.equal(acts2, acts[:B, 1])
    out = _sent(B + 1)
    ops.sample_probs(p32.to(DEV).contiguous(), ud, out[:B])
    assert torch.equal(out[:B].cpu(), want.float()) and _is_sent(out[B:])


def test_samplers_on_rows_built_to_be_exact():
    """dyadic probabilities (every running sum exact): u on a boundary picks the boundary's action (cs >= u); u above the
    last running sum is -1 from a2c_sample_probs and A - 1 from a2c_softmax_sample; one-hot rows; A = 1"""
    ops = _ops()
    q = torch.full((4, 4), 0.25)
    u = torch.tensor([0.0, 0.25, 0.5, 1.0])
    out = _sent(4)
    ops.sample_probs(q.to(DEV), u.to(DEV), out)
    assert out.cpu().tolist() == [0.0, 0.0, 1.0, 3.0]
    assert O.sample_action(q, u).tolist() == [0.0, 0.0, 1.0, 3.0]
    # u above the running sum: a short row (sum 0.875), and a full row with u > 1
    p = torch.tensor([[0.25, 0.25, 0.25, 0.125], [0.25, 0.25, 0.25, 0.25], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 1.0, 0.0],
                      [1.0, 0.0, 0.0, 0.0]])
    u = torch.tensor([0.9, 1.5, 0.3, 1.0, 0.0])
    out = _sent(5)
    ops.sample_probs(p.to(DEV), u.to(DEV), out)
    assert out.cpu().tolist() == [-1.0, -1.0, 2.0, 2.0, 0.0] == O.sample_action(p, u).tolist()
    # softmax_sample: equal logits are p = 1/4 each exactly; a logit GAP above the rest is a one-hot row
    lg = torch.zeros(8, 4)
    lg[5, 2] = GAP
    lg[6, 0] = GAP
    lg[7, 3] = GAP
    u = torch.tensor([0.0, 0.25, 0.5, 1.0, 1.5, 0.3, 0.0, 0.999])
    acts = torch.full((8,), -7, dtype=torch.int64, device=DEV)
    probs = _sent(8, 4)
    ops.softmax_sample(lg.to(DEV), u.to(DEV), acts.data_ptr(), 1, 8, 4, probs=probs)
    assert acts.cpu().tolist() == [0, 0, 1, 3, 3, 2, 0, 3]
    assert torch.equal(probs.cpu(), F.softmax(lg, -1)) and probs[5].cpu().tolist() == [0.0, 0.0, 1.0, 0.0]
    # A = 1: always action 0, also past the sum
    one = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    ops.softmax_sample(torch.tensor([[0.3], [-2.0], [9.0]], device=DEV), torch.tensor([0.0, 0.7, 1.5], device=DEV), one.data_ptr(), 1, 3, 1)
    assert one.cpu().tolist() == [0, 0, 0]
    out = _sent(3)
    ops.sample_probs(torch.ones(3, 1, device=DEV), torch.tensor([0.0, 1.0, 1.5], device=DEV), out)
    assert out.cpu().tolist() == [0.0, 0.0, -1.0]


# ====================================================================================================== column sums
@pytest.mark.parametrize("N", [1, 255, 256, 257, 2000])
@pytest.mark.parametrize("M", [0, 1, 7, 300, 32768])
def test_colsum_vs_fp64(M, N):
    """a2c_colsum over the rows of a wider buffer (ld > N) against the fp64 column sums; M = 0 gives zeros"""
    ops = _ops()
    x = _nrm((M, N + 3), 7000 + M + N)
    xd = x.to(DEV)
    ws = torch.empty(max(1, ops.colsum_ws_bytes(N) // 4), device=DEV)
    out = _sent(N + 2)
    ops.colsum(xd.data_ptr() if M else 0, N + 3, M, N, out[:N], ws)
    assert _is_sent(out[N:])
    if M == 0:
        assert bool((out[:N] == 0).all())
    else:
        _crit("colsum", out[:N], _running_sum(x[:, :N]), x[:, :N].double().sum(0), float(x[:, :N].abs().max()))
    if N > 1:
        _raises(ERR_WORKSPACE, ops.colsum, xd.data_ptr(), N + 3, M, N, _sent(N), ws[:ws.numel() - 1])


# ====================================================================================================== composed head
SN_MAX = 8


@pytest.mark.parametrize("F_", [1, 31, 33, 2592])
@pytest.mark.parametrize("H", [1, 200, 256])
@pytest.mark.parametrize("N", [1, 3, 7, SN_MAX])
def test_compose_heads_vs_fp64(N, H, F_):
    """a2c_compose_heads (models.py:73, 84-85 composed for inference): Wc = Wh Wp, bc = Wh bp + bh"""
    ops = _ops()
    seed = 8000 + N + H + F_
    Wh, bh, Wp, bp = _u((N, H), seed), _u((N,), seed + 1), _u((H, F_), seed + 2) * 0.1, _u((H,), seed + 3) * 0.1
    # the two torch runs also cover 64 pool heads (rows of Wh) the kernel does not see
    Whp, bhp = torch.cat([Wh, _u((64, H), seed + 4)]), torch.cat([bh, _u((64,), seed + 5)])
    Wc, bc = _sent(N + 1, F_), _sent(N + 1)
    ops.compose_heads(Wh.to(DEV), bh.to(DEV), Wp.to(DEV), bp.to(DEV), Wc[:N], bc[:N])
    assert _is_sent(Wc[N:]) and _is_sent(bc[N:])
    term = float(Wh.abs().max() * Wp.abs().max())
    _crit("compose_heads.Wc", Wc[:N], Whp @ Wp, Whp.double() @ Wp.double(), term)
    _crit("compose_heads.bc", bc[:N], Whp @ bp + bhp, Whp.double() @ bp.double() + bhp.double(),
          max(float(Wh.abs().max() * bp.abs().max()), float(bh.abs().max())))


def test_compose_heads_refuses_more_than_sn_max_heads():
    ops = _ops()
    N, H, F_ = SN_MAX + 1, 16, 8
    Wc, bc = _sent(N, F_), _sent(N)
    _raises(ERR_ARG, ops.compose_heads, torch.zeros(N, H, device=DEV), torch.zeros(N, device=DEV), torch.zeros(H, F_, device=DEV),
            torch.zeros(H, device=DEV), Wc, bc)
    assert _is_sent(Wc) and _is_sent(bc)


# ====================================================================================================== split-K slabs
@pytest.mark.parametrize("splitk", [1, 4, 32])
@pytest.mark.parametrize("M,N,K", [(5, 3, 7), (130, 257, 100), (8, 1030, 4104)])
@pytest.mark.parametrize("tA,tB", [(0, 1), (0, 0), (1, 0), (1, 1)])
def test_gemm_partial_slabs_sum_to_the_product(tA, tB, M, N, K, splitk):
    """a2c_gemm_f32_partial: a2c_gemm_splits(K, splitk) slabs [M][N] whose fp64 sum is the product; nothing behind them"""
    ops = _ops()
    from a2c_amd import _lib
    A, B = _u((K, M) if tA else (M, K), 9000 + K), _u((N, K) if tB else (K, N), 9001 + K)
    a64 = A.double().t() if tA else A.double()
    b64 = B.double().t() if tB else B.double()
    a32 = A.t() if tA else A
    b32 = B.t() if tB else B
    splits = _lib.load().a2c_gemm_splits(K, splitk)
    assert 1 <= splits <= splitk
    ws = _sent(splits * M * N + 64)
    Ad, Bd = A.to(DEV), B.to(DEV)
    got = ops.gemm_partial(tA, tB, M, N, K, Ad.data_ptr(), A.shape[1], Bd.data_ptr(), B.shape[1], splitk, ws)
    assert got == splits and _is_sent(ws[splits * M * N:])
    slabs = ws[:splits * M * N].view(splits, M, N).cpu().double().sum(0)
    _crit("gemm_partial", slabs, _running_mm(a32, b32), a64 @ b64, float(A.abs().max() * B.abs().max()))
    if splits * M * N > 1:
        _raises(ERR_WORKSPACE, ops.gemm_partial, tA, tB, M, N, K, Ad.data_ptr(), A.shape[1], Bd.data_ptr(), B.shape[1], splitk,
                ws[:splits * M * N - 1])


# ====================================================================================================== unpack_bits / rollout_post_u8
@pytest.mark.parametrize("n,n_pixels,src_stride,dst_stride", [(1, 16, 2, 16), (5, 7056, 882, 7056), (3, 7056, 900, 7072), (2, 4112, 514, 4128)])
def test_unpack_bits_vs_numpy(n, n_pixels, src_stride, dst_stride):
    """a2c_unpack_bits against numpy.unpackbits (little bit order, as the packed transport writes it); strided rows on both
    sides, the gaps untouched"""
    ops = _ops()
    px = (np.random.default_rng(n_pixels + n).random((n, n_pixels)) < 0.4).astype(np.uint8)
    packed = np.packbits(px, axis=1, bitorder="little")
    assert packed.shape[1] == n_pixels // 8
    src = np.full((n, src_stride), 0xA5, np.uint8)
    src[:, :n_pixels // 8] = packed
    assert np.array_equal(np.unpackbits(src[:, :n_pixels // 8], axis=1, bitorder="little"), px)
    sd = torch.from_numpy(src).to(DEV)
    dst = torch.full((n + 1, dst_stride), 77, dtype=torch.uint8, device=DEV)
    ops.unpack_bits(sd.data_ptr(), src_stride, dst.data_ptr(), dst_stride, n, n_pixels)
    got = dst.cpu().numpy()
    assert np.array_equal(got[:n, :n_pixels], px)
    assert (got[:n, n_pixels:] == 77).all() and (got[n:] == 77).all()


def test_unpack_bits_refuses_a_ragged_pixel_count():
    ops = _ops()
    sd = torch.zeros(4, 64, dtype=torch.uint8, device=DEV)
    dst = torch.full((4, 64), 77, dtype=torch.uint8, device=DEV)
    for n_pixels in (8, 20, 28):          # not a multiple of 16
        _raises(ERR_ARG, ops.unpack_bits, sd.data_ptr(), 64, dst.data_ptr(), 64, 4, n_pixels)
    _raises(ERR_ARG, ops.unpack_bits, sd.data_ptr(), 2, dst.data_ptr(), 64, 4, 32)          # source rows shorter than the bits
    _raises(ERR_ARG, ops.unpack_bits, sd.data_ptr(), 64, dst.data_ptr(), 16, 4, 32)         # destination rows too short
    assert bool((dst == 77).all())


@pytest.mark.parametrize("t", [0, 2])
def test_rollout_post_u8_equals_rollout_post_on_the_same_frames(t):
    """a2c_rollout_post_u8 (runner.py:199-232, uint8 frames at a padded stride) against a2c_rollout_post on the same frames
    as floats: every output bit for bit"""
    ops = _ops()
    B, T, slot0, n_slots, C, HW = 7, 5, 1, 9, 4, 84 * 84
    S = C * HW
    gamma = 0.99
    mk = lambda: dict(rw=_u((n_slots * T,), 50).to(DEV), dn=(_u((n_slots * T,), 51, 0, 1) < 0.3).float().to(DEV),
                      dl=_u((n_slots * T,), 52).to(DEV), vp=_u((B,), 53).to(DEV), states=_u((n_slots * T, S), 57, 0, 1).to(DEV))
    rew = torch.tensor([0., 1, -1, 0, 0, 2, 0]).to(DEV)
    done = torch.tensor([0., 0, 0, 1, 0, 0, 1]).to(DEV)
    val = _u((B, 4), 55).to(DEV)
    fs = HW + 16
    f8 = torch.full((B, fs), 9, dtype=torch.uint8, device=DEV)
    f8[:, :HW] = (_u((B, HW), 59, 0, 1) < 0.3).to(torch.uint8).to(DEV)
    f32 = f8[:, :HW].float().contiguous()
    sp = lambda D, k: D["states"].data_ptr() + 4 * (slot0 * T + k) * S
    a, b = mk(), mk()
    ops.rollout_post(rew, done, val.data_ptr() + 12, 4, a["vp"], a["rw"], a["dn"], a["dl"], T, t, slot0, gamma, True, f32, done,
                     sp(a, t), T * S, sp(a, t + 1), T * S, B, C, HW)
    ops.rollout_post_u8(rew, done, val.data_ptr() + 12, 4, b["vp"], b["rw"], b["dn"], b["dl"], T, t, slot0, gamma, True,
                        f8.data_ptr(), fs, done, sp(b, t), T * S, sp(b, t + 1), T * S, B, C, HW)
    fresh = mk()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["states"], fresh["states"]) and not torch.equal(a["rw"], fresh["rw"])
    nxt = a["states"].view(n_slots, T, C, HW)[slot0:slot0 + B, t + 1]
    assert torch.equal(nxt[:, C - 1], f32)
