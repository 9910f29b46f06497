"""-m gpu: the generic convolution kernels of csrc/conv.hip at the layer shapes the device worlds feed them -- A3CModel,
ConvModel and GRUModel on 80 x 80 (Pong-device), 80 x 72 (Breakout-device) and 60 x 60 (Snake-device) frames -- and at a few
synthetic shapes for the instantiations no model layer reaches.  The case list is CASES of tests/test_conv_routes.py, whose
CPU twin of the dispatcher says which kernel each case runs and that every launched instantiation has a case.

Every result goes against F.conv2d and autograd in fp64 on the CPU (computed once per spec at B = 5; B = 1 is its first
sample), with the tolerances tests/test_gpu_kernels.py::test_conv2d_fwd_bwd holds these kernels to: 2e-6 + 1e-5 |want| for
the forward and backward-data, 1e-5 max|want| + 1e-5 |want| for the gradients.  TOL holds what a case needs beyond that,
as (measured error of the plain fp32 CPU convolution against the same fp64 reference, factor 2); it is empty: no case
needed more.  Each figure is printed before it is asserted (`pytest -s`).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import a2c_oracle as O  # noqa: E402
from cases import hashf  # noqa: E402
from test_conv_routes import BATCHES, CASES, PERSISTENT, PERSISTENT_B, UNALIGNED, case_routes  # noqa: E402
from test_gpu_kernels import DEV, _ops, close, rnd  # noqa: E402

torch.set_num_threads(4)

FWD_TOL = (2e-6, 1e-5)          # atol, rtol
GRAD_TOL = 1e-5                 # of max|want|, plus 1e-5 relative
# (spec, B, what) -> (max error of the fp32 CPU convolution against fp64 at that case, factor): the kernel may be off by
# factor x that error.  No case needed an entry.
TOL = {}

_REF = {}


def reference(spec):
    """inputs as in test_conv2d_fwd_bwd and their fp64 results, B = max(BATCHES) samples; computed once per spec"""
    if spec in _REF:
        return _REF[spec]
    Cin, H, W, Cout, ks, s, p = spec
    B = max(BATCHES)
    x = rnd((B, Cin, H, W), 90, 0, 1)
    w = rnd((Cout, Cin, ks, ks), 91) / (Cin * ks * ks) ** 0.5
    bias = rnd((Cout,), 92) * 0.1
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, bias))
    pre = F.conv2d(xr, wr, br, stride=s, padding=p)
    y = F.relu(pre).detach()
    gpre = (rnd(tuple(y.shape), 93).double() * (pre.detach() > 0)).float()        # dOut as the kernels get it (fp32)
    pre.backward(gpre.double())
    r = dict(x=x, w=w, bias=bias, y=y, gpre=gpre, dx=xr.grad.clone(), dW={B: wr.grad.clone()}, db={B: br.grad.clone()})
    for b in BATCHES:
        if b != B:          # the gradient of the first b samples alone
            w1, b1 = w.double().requires_grad_(True), bias.double().requires_grad_(True)
            F.conv2d(x[:b].double(), w1, b1, stride=s, padding=p).backward(gpre[:b].double())
            r["dW"][b], r["db"][b] = w1.grad, b1.grad
    _REF[spec] = r
    return r


def check(name, got, want, atol, rtol, key=None):
    g, wnt = got.detach().cpu().double(), want.double()
    err = float((g - wnt).abs().max())
    if key in TOL:
        atol = max(atol, TOL[key][0] * TOL[key][1])
    print(f"  {name}: max |err| {err:.3e}, scale {float(wnt.abs().max()):.3g}, atol {atol:.3e}")
    close(name, got, want, atol, rtol)


def check_grad(name, got, want, key=None):
    check(name, got, want, GRAD_TOL * float(want.abs().max()), 1e-5, key)


class Layer:
    """one spec on the device: prepared weights and the three calls, every output pre-filled with NaN"""

    def __init__(self, spec):
        self.ops, self.spec = _ops(), spec
        self.d = self.ops.conv_desc(*spec)
        Cin, H, W, Cout, ks, s, p = spec
        self.n_in, self.n_out = Cin * H * W, Cout * self.d.OH * self.d.OW
        r = reference(spec)
        self.w, self.bias = r["w"].to(DEV), r["bias"].to(DEV)
        self.wf = torch.empty(self.ops.conv_prep_floats(self.d, 0), device=DEV)
        self.wb = torch.empty(self.ops.conv_prep_floats(self.d, 1), device=DEV)
        self.ops.conv_prep(self.d, 0, self.w, self.wf)
        self.ops.conv_prep(self.d, 1, self.w, self.wb)

    def rows(self, x, pad):
        """x (B, ...) as rows of a wider buffer: sample stride n_in + pad floats"""
        B = x.shape[0]
        buf = torch.full((B, self.n_in + pad), float("nan"), device=DEV)
        buf[:, :self.n_in] = x.reshape(B, -1).to(DEV)
        return buf

    def fwd(self, xbuf, B, gap=4):
        """-> (B, Cout, OH, OW) out of a NaN-filled buffer whose rows are n_out + gap floats apart; the gap must stay NaN"""
        obuf = torch.full((B, self.n_out + gap), float("nan"), device=DEV)
        self.ops.conv_fwd(self.d, xbuf.data_ptr(), xbuf.stride(0), self.wf, self.bias, True, obuf.data_ptr(), B,
                          out_bstride=obuf.stride(0))
        assert torch.isnan(obuf[:, self.n_out:]).all(), "forward wrote between the output rows"
        return obuf[:, :self.n_out].reshape(B, self.spec[3], self.d.OH, self.d.OW)

    def bwd_data(self, dout, mask, B):
        din = torch.full((B,) + tuple(self.spec[:3]), float("nan"), device=DEV)
        self.ops.conv_bwd_data(self.d, dout, self.wb, mask, din, B)
        return din

    def bwd_weight(self, xbuf, dout, B):
        dW, db = torch.full_like(self.w, float("nan")), torch.full_like(self.bias, float("nan"))
        ws = torch.empty(max(4, self.ops.conv_bwd_weight_ws_bytes(self.d, B)) // 4, device=DEV)
        self.ops.conv_bwd_weight(self.d, xbuf.data_ptr(), xbuf.stride(0), dout, dW, db, B, ws)
        return dW, db


def offset_by_one_float(t):
    """a copy of t on the device that starts 4 bytes behind a 16-byte boundary"""
    buf = torch.full((t.numel() + 8,), float("nan"), device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


SPECS = [c["spec"] for c in CASES]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("spec", SPECS, ids=str)
def test_world_layer_against_fp64(spec, B, monkeypatch):
    """forward (bias, ReLU, strided input rows, strided output rows), backward-data with a float mask and without, weight
    and bias gradient -- at default switches, and the forward once more with the tile tuner off (the route the twin names;
    the tuner may settle on another tile budget, and under a small one a row-run layer runs the generic kernel)"""
    L, r = Layer(spec), reference(spec)
    f, b, w = case_routes(spec)
    print(f"\n  {spec} B={B}: {f} | {b} | {w}")
    x, gpre = r["x"][:B], r["gpre"][:B]
    xbuf = L.rows(x, 8)
    check("fwd", L.fwd(xbuf, B), r["y"][:B], *FWD_TOL, key=(spec, B, "fwd"))
    monkeypatch.setenv("A2C_NO_TUNE", "1")
    check("fwd, tuner off", L.fwd(xbuf, B), r["y"][:B], *FWD_TOL, key=(spec, B, "fwd"))
    monkeypatch.delenv("A2C_NO_TUNE")
    dout = gpre.contiguous().to(DEV)
    mask = (x - 0.5).to(DEV)          # the ReLU mask of the layer below: x > 0.5
    check("bwd_data, mask", L.bwd_data(dout, mask, B), r["dx"][:B] * (x > 0.5), *FWD_TOL, key=(spec, B, "bwd_data"))
    check("bwd_data, no mask", L.bwd_data(dout, None, B), r["dx"][:B], *FWD_TOL, key=(spec, B, "bwd_data"))
    if w == "ERR_ARG":          # more k-tiles than plan_wgrad's ladder has: refused, nothing launched
        with pytest.raises(RuntimeError, match="a2c_conv2d_bwd_weight"):
            L.bwd_weight(xbuf, dout, B)
        assert L.ops.conv_bwd_weight_ws_bytes(L.d, B) == 0
        return
    dW, db = L.bwd_weight(xbuf, dout, B)
    check_grad("bwd_weight", dW, r["dW"][B], key=(spec, B, "bwd_weight"))
    check_grad("bwd_bias", db, r["db"][B], key=(spec, B, "bwd_bias"))


@pytest.mark.parametrize("spec, what", list(UNALIGNED), ids=str)
def test_unaligned_entry_against_fp64(spec, what):
    """`bstride`: input rows one float more than a multiple of four apart (every sample but the first starts off a 16-byte
    boundary): the generic forward kernel with scalar staging and the weight gradient without `run` / prefetch.  `dout`: dOut
    starts one float behind a 16-byte boundary: scalar staging in backward-data and in the weight gradient"""
    B = max(BATCHES)
    L, r = Layer(spec), reference(spec)
    print(f"\n  {spec} {what}: " + " | ".join(x for x in case_routes(spec, what) if x))
    x, gpre = r["x"], r["gpre"]
    dout = gpre.contiguous().to(DEV)
    if what == "bstride":
        xbuf = L.rows(x, 9)
        assert xbuf.stride(0) % 4 == 1
        check("fwd", L.fwd(xbuf, B), r["y"], *FWD_TOL, key=(spec, what, "fwd"))
        check("fwd, odd output rows", L.fwd(xbuf, B, gap=5), r["y"], *FWD_TOL, key=(spec, what, "fwd"))
    else:
        xbuf = L.rows(x, 8)
        dout = offset_by_one_float(dout)
        mask = (x - 0.5).to(DEV)
        check("bwd_data, mask", L.bwd_data(dout, mask, B), r["dx"] * (x > 0.5), *FWD_TOL, key=(spec, what, "bwd_data"))
        check("bwd_data, no mask", L.bwd_data(dout, None, B), r["dx"], *FWD_TOL, key=(spec, what, "bwd_data"))
    dW, db = L.bwd_weight(xbuf, dout, B)
    check_grad("bwd_weight", dW, r["dW"][B], key=(spec, what, "bwd_weight"))
    check_grad("bwd_bias", db, r["db"][B], key=(spec, what, "bwd_bias"))


@pytest.mark.parametrize("spec", list(PERSISTENT), ids=str)
def test_more_tiles_than_workgroups(spec, monkeypatch):
    """B = 320, sample i = sample i % 5 of the B = 5 case: the persistent loops of resident_grid run several rounds and
    wgrad_reduce_kernel sums a full slab count.  Forward and backward-data rows equal the B = 5 rows of the same sample bit for
    bit with the tile tuners off, and with them on (called twice: the tuning call and the cached one); the gradients are 64 x
    the fp64 B = 5 gradients"""
    B5, B = max(BATCHES), PERSISTENT_B
    L, r = Layer(spec), reference(spec)
    print(f"\n  {spec} B={B}: stands for {PERSISTENT[spec]}")
    idx = torch.arange(B, device=DEV) % B5
    x5, g5 = r["x"].to(DEV), r["gpre"].contiguous().to(DEV)
    x5buf = L.rows(r["x"], 8)
    xbuf = x5buf[idx].contiguous()
    dout, mask5 = g5[idx].contiguous(), x5 - 0.5
    mask = mask5[idx].contiguous()
    monkeypatch.setenv("A2C_NO_TUNE", "1")
    f5, d5 = L.fwd(x5buf, B5), L.bwd_data(g5, mask5, B5)
    check("fwd B=5", f5, r["y"], *FWD_TOL)
    check("bwd_data B=5", d5, r["dx"] * (r["x"] > 0.5), *FWD_TOL)
    assert torch.equal(L.fwd(xbuf, B), f5[idx]), "forward rows differ between B = 5 and B = 320 (tuner off)"
    assert torch.equal(L.bwd_data(dout, mask, B), d5[idx]), "backward-data rows differ between B = 5 and B = 320 (tuner off)"
    monkeypatch.delenv("A2C_NO_TUNE")
    for call in (1, 2):
        assert torch.equal(L.fwd(xbuf, B), f5[idx]), f"forward rows differ with the tuner on (call {call})"
        assert torch.equal(L.bwd_data(dout, mask, B), d5[idx]), f"backward-data rows differ with the tuner on (call {call})"
    dW, db = L.bwd_weight(xbuf, dout, B)
    check_grad("bwd_weight", dW, (B // B5) * r["dW"][B5])
    check_grad("bwd_bias", db, (B // B5) * r["db"][B5])


@pytest.mark.parametrize("kind", ["A3CModel", "ConvModel", "GRUModel"])
def test_model_gradients_on_a_breakout_frame_against_fp64(kind):
    """forward and every parameter gradient through the public autograd bridge at state shape (4, 80, 72), batch 3, against
    O.OracleNet run in fp64 (OracleNet and formula_state_dict take the non-square frame as it is): the method and the
    tolerances of test_gpu_models.py::test_model_forward_golden_and_grads, without golden files"""
    import a2c_amd
    ss, A, h, B = (4, 80, 72), 4, 64, 3
    sd = O.formula_state_dict(kind, ss, A, h)
    net = getattr(a2c_amd.models, kind)(list(ss), A, h_size=h, bnorm=False)
    assert set(net.state_dict().keys()) == set(sd.keys())
    net.load_state_dict(sd)
    onet = O.OracleNet(kind, ss, A, h, state_dict={k: v.double() if v.is_floating_point() else v for k, v in sd.items()})
    x = torch.from_numpy(O.formula_frames(B, ss, seed=700, binary=False))
    gv = torch.from_numpy(hashf(B, 710, -1, 1).reshape(B, 1))
    gp = torch.from_numpy(hashf(B * A, 720, -1, 1).reshape(B, A))
    gh = torch.from_numpy(hashf(B * h, 730, -1, 1).reshape(B, h))
    hin = torch.from_numpy(hashf(B * h, 740, -1, 1).reshape(B, h)) if net.is_recurrent else None
    if net.is_recurrent:
        hin_o = hin.double().requires_grad_(True)
        out_o = onet(x.double(), hin_o)
    else:
        out_o = onet(x.double())
    sum((o * g.double()).sum() for o, g in zip(out_o, (gv, gp, gh))).backward()
    with torch.no_grad():          # (as in that test: the first call builds the parameter arena, which points every p.grad at
        out = net(x, hin) if net.is_recurrent else net(x)      # its gradient slice; autograd must start from no .grad)
    for name, o, oo in zip(("val", "pi", "h"), out, out_o):
        check(name + " (no grad)", o, oo.detach(), 1e-5, 1e-5)
    net.req_grads(True)
    for q in net.parameters():
        q.grad = None
    if net.is_recurrent:
        hin_d = hin.to(DEV).requires_grad_(True)
        out = net(x, hin_d)
    else:
        out = net(x)
    sum((o * g.to(DEV)).sum() for o, g in zip(out, (gv, gp, gh))).backward()
    for name, o, oo in zip(("val", "pi", "h"), out, out_o):
        check(name, o, oo.detach(), 1e-5, 1e-5)
    if net.is_recurrent:
        check("d h_in", hin_d.grad, hin_o.grad, 1e-6, 1e-4)
    for (n, q), (n2, q2) in zip(net.named_parameters(), onet.named_parameters()):
        assert n == n2
        if q2.grad is None:
            assert q.grad is None or float(q.grad.abs().max()) == 0.0, n
            continue
        scale = float(q2.grad.abs().max()) + 1e-12
        check(f"grad {n}", q.grad, q2.grad, 2e-5 * scale, 2e-5)
