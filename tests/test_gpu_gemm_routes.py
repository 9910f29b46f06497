"""-m gpu: every dispatch route of a2c_gemm_f32 / a2c_gemm_f32_partial / a2c_gemm_x6_images (csrc/gemm.hip) at its edge
shapes against fp64.  The cases and the route each one takes come from tests/test_gemm_routes.py (`CASES`, checked there on
the CPU against the text of the dispatcher); here every case runs once through a2c_amd.ops.

Per case: operands uniform in [-1, 1) at full fp32 resolution (`_u`), A and B as views of larger random buffers (lda / ldb
beyond the row, a row behind the last: a kernel that reads past K or past the last row reads other numbers, not zeros),
C with ldc > N where the route allows it and rows behind M, C, the slabs and the workspace filled with a sentinel that must
be intact everywhere outside [M, N] and behind the workspace.  Reference: float64 A @ B on the CPU with the epilogue in
the kernel's order (accumulate, bias, ReLU, mask > 0; half the mask entries <= 0 with exact zeros and a -0.0 among them).
Criterion: `_crit` of test_gpu_small_kernels, e_k <= 2 e_t + ulp(scale), e_t the error of `_running_mm` (fp32 products
and additions in k order) over the whole output against the same fp64 reference, scale = max|a| max|b| raised to max|bias| /
max|C0| where those enter.  Outputs of fewer than 4096 elements borrow further rows of the same distribution for e_t (the
kernel sees the first M), as the small-kernel tests do.  The x 6 routes assert what the project accepts for that path --
rms error against fp64 at most 1.5 x (+ 1e-7 of the rms) that of the fp32 route on the same call -- and print their
e_k / e_t.  Bit for bit: the same call twice, on every route; a2c_gemm_f32 with split K against a2c_gemm_f32_partial + the
fp32 slab sum in slab order + the epilogue, wherever both take the same slab kernel (gemm_nt / skinny_stream against
gemm_kernel are equal only up to summation order: nothing is asserted there).

Left out: gemm_nt<Big> at M = 256 and the M = 256 / 257 edge -- N K >= 2^22 puts M N K at 1.07e9 there, over the 3e8 the
running-sum reference is held to; test_gemm_rollout_batch_forward_...[256] runs that shape at 73 tiles per split.

Worst e_k / e_t per route measured on an MI355X over all cases of this file (`pytest -s` prints them at the end; "+reduce":
the epilogue ran in splitk_reduce_kernel): gemm_kernel 1.60 with M <= 96 and 1.29 above it (1.31 / 1.29 +reduce), the same in
all four orientations; small_gemm_kernel<*, 4> 0.75 / 0.66 (B k- / n-contiguous), <*, 8> 0.29; small_n_fwd 1.00,
small_n_bwd_data 1.00, small_n_bwd_weight 1.32, small_k_tn<4> 0.97, <1> 0.96; gemm_nt<Skinny> 0.26, gemm_nt<Big> 0.27,
skinny_stream<1> 0.26, <2> 0.23 (their slabs alone 0.04 - 0.09: a split sums few terms); the x 6 route, printed and not
asserted, 1.10, its rms error 0.60 - 1.17 x the fp32 route's.  474 cases; wall time of the file inside a run of the whole suite: 8.3 s of test calls (test_gpu_conv3.py: 43 s); 15.5 s on
its own.
"""
import functools
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gemm_routes as R  # noqa: E402
from test_gpu_small_kernels import DEV, ERR_ARG, ERR_WORKSPACE, SENT, _crit, _ops, _raises, _running_mm, _sent, _u  # noqa: E402

_RATIOS = {}
_T0 = [None]
SWITCHES = ("A2C_GEMM_X9", "A2C_NO_GEMM_NT", "A2C_NO_SKINNY_STREAM")
POOL_ELEMS = 4096


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    _T0[0] = time.time()
    yield
    print(f"\nworst e_k / e_t per route over this run ({time.time() - _T0[0]:.1f} s):")
    for k in sorted(_RATIOS):
        print(f"  RATIO {k} {_RATIOS[k]:.3f}")


def _seed(*a):
    s = 17
    for x in a:
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=16)
def _reference(M, N, K):
    """-> a [Mref][K], b [K][N] (fp32, logical), a @ b in fp64 and as the fp32 running sum over k, max|a| max|b|.  Shared by
    every case of the same M, N, K, whatever its orientation, leading dimensions and epilogue."""
    Mref = max(M, -(-POOL_ELEMS // max(N, 1)))
    a, b = _u((Mref, K), _seed(1, M, N, K)), _u((K, N), _seed(2, M, N, K))
    t64 = a.double() @ b.double()
    t32 = _running_mm(a, b)
    scale = float(a.abs().max() * b.abs().max()) if a.numel() and b.numel() else 0.0
    return a, b, t64, t32, scale


@functools.lru_cache(maxsize=16)
def _epilogue_inputs(M, N, K):
    Mref = _reference(M, N, K)[0].shape[0]
    C0, bias, mask = _u((Mref, N), _seed(3, M, N, K)), _u((N,), _seed(4, M, N, K)), _u((Mref, N), _seed(5, M, N, K))
    mf = mask.reshape(-1)
    if mf.numel():
        mf[::7] = 0.0                   # exact zeros and a -0.0 among the entries <= 0
        mf[mf.numel() // 2] = -0.0
    return C0, bias, mask


def _epilogue(pre, C0, bias, mask, c, dtype):
    """the kernel's order: accumulate, bias, ReLU, mask > 0"""
    v = pre.to(dtype)
    if c["acc"]:
        v = v + C0.to(dtype)
    if c["bias"]:
        v = v + bias.to(dtype)
    if c["relu"]:
        v = torch.relu(v)
    if c["mask"]:
        v = torch.where(mask > 0, v, torch.zeros((), dtype=dtype))
    return v


def _embed(logical, ld, off, seed):
    """a device buffer of random numbers holding `logical` [rows][cols] at float offset `off` with leading dimension ld, one row
    and 8 floats behind it -> (buffer, pointer)"""
    rows, cols = logical.shape
    par = _u((off + (rows + 1) * ld + 8,), seed)
    par[off:off + rows * ld].view(rows, ld)[:, :cols] = logical
    par = par.to(DEV)
    return par, par.data_ptr() + 4 * off


def _c_buffer(M, N, ldc, off, C0):
    """sentinels everywhere: [M + 2][ldc] behind `off` floats, C0 (or nothing) inside [M, N] -> buffer, pointer, inside-mask"""
    n = off + (M + 2) * ldc + 8
    par = torch.full((n,), SENT)
    inside = torch.zeros(n, dtype=torch.bool)
    inside[off:off + M * ldc].view(M, ldc)[:, :N] = True
    if C0 is not None:
        par[off:off + M * ldc].view(M, ldc)[:, :N] = C0[:M]
    par = par.to(DEV)
    return par, par.data_ptr() + 4 * off, inside


def _region(par, M, N, ldc, off):
    return par[off:off + M * ldc].view(M, ldc)[:, :N]


def _record(route, ratio):
    if ratio is not None:
        k = R.family(route) + ("+reduce" if "+reduce" in route else "")
        _RATIOS[k] = max(_RATIOS.get(k, 0.0), ratio)


def _set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _workspace(nb):
    """-> (the tensor the call gets or None, the whole sentinel buffer, floats passed)"""
    n = nb // 4
    buf = _sent(n + 64)
    return (buf[:n] if n > 0 else None), buf, n


class _Call:
    """one case of kind 'gemm' set up on the device; run() makes the call on a fresh C"""

    def __init__(self, c):
        ops = _ops()
        self.c, self.ops = c, ops
        M, N, K = c["M"], c["N"], c["K"]
        self.lda, self.ldb, self.ldc, self.ldm = R.lds(c)
        a, b, self.t64, self.t32, self.scale = _reference(M, N, K)
        self.C0, self.bias, self.mask = _epilogue_inputs(M, N, K)
        A = a[:M].t() if c["tA"] else a[:M]
        B = b.t() if c["tB"] else b
        self.Apar, self.Ap = _embed(A, self.lda, c["oa"], _seed(6, M, N, K))
        self.Bpar, self.Bp = _embed(B, self.ldb, c["ob"], _seed(7, M, N, K))
        self.Mpar, self.Mp = _embed(self.mask[:M], self.ldm, c["om"], _seed(8, M, N, K))
        bp = torch.full((c["obias"] + N + 8,), SENT)
        bp[c["obias"]:c["obias"] + N] = self.bias
        self.bias_par = bp.to(DEV)
        self.bias_dev = self.bias_par[c["obias"]:c["obias"] + N]
        self.nb = R.case_ws_bytes(c)

    def run(self, splitk=None, nb=None):
        c, ops = self.c, self.ops
        M, N, K = c["M"], c["N"], c["K"]
        Cpar, Cp, inside = _c_buffer(M, N, self.ldc, c["oc"], self.C0 if c["acc"] else None)
        ws, wsbuf, n = _workspace(self.nb if nb is None else nb)
        ops.gemm(c["tA"], c["tB"], M, N, K, self.Ap, self.lda, self.Bp, self.ldb, Cp, self.ldc,
                 bias=self.bias_dev if c["bias"] else None, relu=c["relu"], mask_ptr=self.Mp if c["mask"] else 0,
                 ldmask=self.ldm if c["mask"] else 0, accumulate=c["acc"], splitk=c["splitk"] if splitk is None else splitk, ws=ws)
        out = Cpar.cpu()
        assert bool((out[~inside] == SENT).all()), f"{c['id']}: a sentinel outside [M, N] of C was overwritten"
        assert bool((wsbuf[n:] == SENT).all()), f"{c['id']}: a sentinel behind the workspace was overwritten"
        return _region(out, M, N, self.ldc, c["oc"]).clone(), Cpar

    def scale_of(self):
        c, s = self.c, self.scale
        if c["bias"] and self.bias.numel():
            s = max(s, float(self.bias.abs().max()))
        if c["acc"] and self.C0.numel():
            s = max(s, float(self.C0.abs().max()))
        return s

    def refs(self):
        return (_epilogue(self.t32, self.C0, self.bias, self.mask, self.c, torch.float32),
                _epilogue(self.t64, self.C0, self.bias, self.mask, self.c, torch.float64))


def _rel_rms(got, want):
    rms = float(want.pow(2).mean().sqrt())
    return float((got.double() - want).pow(2).mean().sqrt()) / rms


def _check_ws_twin(c):
    """the twin's workspace sizes are the library's"""
    ops = _ops()
    if c["kind"] == "gemm" and c["M"] > 0 and c["N"] > 0:
        assert ops.gemm_ws_bytes(c["M"], c["N"], c["splitk"], c["K"]) == R.full_ws_bytes(c["M"], c["N"], c["K"], c["splitk"], c["env"])
        assert ops.gemm_ws_bytes(c["M"], c["N"], c["splitk"]) == R.ws_bytes(c["M"], c["N"], c["splitk"])


def _run_gemm(c, route, monkeypatch):
    M, N, K = c["M"], c["N"], c["K"]
    call = _Call(c)
    if c["expect"] in ("ERR_ARG", "ERR_WORKSPACE"):
        Cpar, Cp, _ = _c_buffer(M, N, call.ldc, c["oc"], None)
        ws, wsbuf, n = _workspace(call.nb)
        _raises(ERR_ARG if c["expect"] == "ERR_ARG" else ERR_WORKSPACE, call.ops.gemm, c["tA"], c["tB"], M, N, K, call.Ap, call.lda,
                call.Bp, call.ldb, Cp, call.ldc, bias=call.bias_dev if c["bias"] else None, relu=c["relu"],
                mask_ptr=call.Mp if c["mask"] else 0, ldmask=call.ldm if c["mask"] else 0, accumulate=c["acc"], splitk=c["splitk"], ws=ws)
        assert bool((Cpar == SENT).all()) and bool((wsbuf == SENT).all()), "a refused call wrote something"
        return
    got, Cpar = call.run()
    if c["expect"] == "nothing":
        assert bool((Cpar == SENT).all())
        return
    got2, _ = call.run()
    assert torch.equal(got, got2), f"{c['id']}: the same call twice, different bits"
    t32, t64 = call.refs()
    if c["expect"] == "gemm_x6_kernel":
        # the criterion of test_gemm_bf16_x9_path_is_the_fp32_product: against the fp32 MFMA route on the same call
        monkeypatch.setenv("A2C_GEMM_X9", "0")
        got32, _ = call.run()
        want = t64[:M]
        e6, e32 = _rel_rms(got, want), _rel_rms(got32, want)
        e_k, e_t = float((got.double() - want).abs().max()), float((t32.double() - t64).abs().max())
        print(f"    {route}: rms error / rms {e6:.3e} (fp32 route {e32:.3e}); e_k / e_t {e_k / e_t:.3f} (printed, not asserted)")
        assert e6 <= 1.5 * e32 + 1e-7, (c["id"], e6, e32)
        assert not torch.equal(got, got32), "the x 6 kernel did not run"
        _RATIOS["gemm_x6_kernel (not asserted)"] = max(_RATIOS.get("gemm_x6_kernel (not asserted)", 0.0), e_k / e_t)
        return
    _record(route, _crit(R.family(route), got, t32, t64, call.scale_of()))
    if "+reduce" in route and R.family(route) != "gemm_x6_kernel":
        _check_against_partial(c, call, route, got)


def _check_against_partial(c, call, route, got):
    """a2c_gemm_f32 with split K == a2c_gemm_f32_partial + the fp32 slab sum in slab order + the epilogue, bit for bit, where
    both take the same slab kernel"""
    M, N, K = c["M"], c["N"], c["K"]
    splits = R.gemm_splits(K, c["splitk"])
    rp = R.route(c["tA"], c["tB"], M, N, K, call.lda, call.ldb, alA=c["oa"] % 4 == 0, alB=c["ob"] % 4 == 0, splitk=c["splitk"],
                 ws=True, ws_nbytes=splits * M * N * 4, env=c["env"], partial=True)
    assert R.family(rp) == R.family(route), (route, rp)
    ws = _sent(splits * M * N)
    assert call.ops.gemm_partial(c["tA"], c["tB"], M, N, K, call.Ap, call.lda, call.Bp, call.ldb, c["splitk"], ws) == splits
    slabs = ws.view(splits, M, N)
    v = torch.zeros(M, N, device=DEV)
    for z in range(splits):
        v += slabs[z]
    if c["acc"]:
        v += call.C0[:M].to(DEV)
    if c["bias"]:
        v += call.bias.to(DEV)
    if c["relu"]:
        v = torch.clamp_min(v, 0.0)
    if c["mask"]:
        v = torch.where(call.mask[:M].to(DEV) > 0, v, torch.zeros((), device=DEV))
    assert torch.equal(v.cpu(), got), f"{c['id']}: split K through a2c_gemm_f32 and through the slabs differ in bits"


def _run_partial(c, route):
    ops = _ops()
    M, N, K = c["M"], c["N"], c["K"]
    lda, ldb, _, _ = R.lds(c)
    a, b, t64, t32, scale = _reference(M, N, K)
    A = a[:M].t() if c["tA"] else a[:M]
    B = b.t() if c["tB"] else b
    Apar, Ap = _embed(A, lda, c["oa"], _seed(6, M, N, K))
    Bpar, Bp = _embed(B, ldb, c["ob"], _seed(7, M, N, K))
    splits = R.gemm_splits(K, c["splitk"])
    lib_splits = None
    outs = []
    for _ in range(2):
        ws = _sent((splits + 1) * M * N + 64)          # room for one slab more than is written
        lib_splits = ops.gemm_partial(c["tA"], c["tB"], M, N, K, Ap, lda, Bp, ldb, c["splitk"], ws)
        assert lib_splits == splits
        assert bool((ws[splits * M * N:] == SENT).all()), "the slab behind the last one was written"
        assert bool((ws[:splits * M * N] != SENT).all()), "an element of a slab was not written"
        outs.append(ws[:splits * M * N].view(splits, M, N).cpu())
    assert torch.equal(outs[0], outs[1])
    _record(route, _crit(R.family(route) + "(partial)", outs[0].double().sum(0), t32, t64, scale))
    if splits * M * N > 1:
        _raises(ERR_WORKSPACE, ops.gemm_partial, c["tA"], c["tB"], M, N, K, Ap, lda, Bp, ldb, c["splitk"], _sent(splits * M * N - 1))


def _run_x6_images(c, route, monkeypatch):
    """tA / tB say how the sources lie, as for a2c_gemm_f32: tA = 0 and tB = 1 are the k-contiguous ones"""
    ops = _ops()
    M, N, K = c["M"], c["N"], c["K"]
    call = _Call(c)
    ia = torch.empty(ops.gemm_x6_image_bytes(M, K) // 2, dtype=torch.int16, device=DEV)
    ib = torch.empty(ops.gemm_x6_image_bytes(N, K) // 2, dtype=torch.int16, device=DEV)
    ops.gemm_x6_split(call.Ap, call.lda, M, K, c["tA"] == 0, ia)
    ops.gemm_x6_split(call.Bp, call.ldb, N, K, c["tB"] != 0, ib)
    outs = []
    for _ in range(2):
        Cpar, Cp, inside = _c_buffer(M, N, call.ldc, c["oc"], call.C0 if c["acc"] else None)
        ws, wsbuf, n = _workspace(call.nb)
        ops.gemm_x6_images(M, N, K, ia, ib, Cp, call.ldc, bias=call.bias_dev if c["bias"] else None, relu=c["relu"],
                           mask_ptr=call.Mp if c["mask"] else 0, ldmask=call.ldm if c["mask"] else 0, accumulate=c["acc"],
                           splitk=c["splitk"], ws=ws)
        out = Cpar.cpu()
        assert bool((out[~inside] == SENT).all()) and bool((wsbuf[n:] == SENT).all())
        outs.append(_region(out, M, N, call.ldc, c["oc"]).clone())
    assert torch.equal(outs[0], outs[1])
    monkeypatch.setenv("A2C_GEMM_X9", "0")
    got32, _ = call.run(splitk=1, nb=0)
    t32, t64 = call.refs()
    want = t64[:M]
    e6, e32 = _rel_rms(outs[0], want), _rel_rms(got32, want)
    e_k, e_t = float((outs[0].double() - want).abs().max()), float((t32.double() - t64).abs().max())
    print(f"    {route} (images): rms error / rms {e6:.3e} (fp32 route {e32:.3e}); e_k / e_t {e_k / e_t:.3f} (printed, not asserted)")
    assert e6 <= 1.5 * e32 + 1e-7, (c["id"], e6, e32)
    if c["splitk"] > 1:
        Cpar, Cp, _ = _c_buffer(M, N, call.ldc, c["oc"], None)
        _raises(ERR_WORKSPACE, ops.gemm_x6_images, M, N, K, ia, ib, Cp, call.ldc, splitk=c["splitk"],
                ws=_sent(c["splitk"] * M * N - 1))
        assert bool((Cpar == SENT).all())


@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES])
def test_gemm_route_vs_fp64(cid, monkeypatch):
    c = R.BY_ID[cid]
    route = R.case_route(c)
    assert R.family(route) == c["expect"]
    print(f"\n  {cid}: {route}")
    _set_env(monkeypatch, c["env"])
    _check_ws_twin(c)
    if c["kind"] == "partial":
        _run_partial(c, route)
    elif c["kind"] == "x6img":
        _run_x6_images(c, route, monkeypatch)
    else:
        _run_gemm(c, route, monkeypatch)
    torch.cuda.synchronize()
