"""-m gpu: the one-launch A3C step kernel (a2c_a3c_step) and both bodies of the persistent rollout (a2c_a3c_rollout: the ring
kernel and, with A2C_NO_RING=1, the per-step body) at the frame shapes of tests/test_step_shapes.py -- ragged conv1 tiles,
every split of the ring's conv2 loop, rows without a stash, without lane masks, without uint8 frames, the LDS edge.
  * a2c_a3c_step against the same chain written out in torch float64 on the CPU (no a2c_amd op in the reference): state
    row, stash, heads, sampled actions, bookkeeping, refusals;
  * Runner rollouts over a process env pool against the CPU oracle, uint8 / packed transport, frame store + lazy states;
  * rollout -> update -> rollout against the oracle, and the update from the stash against the recomputed one.
Tolerances are the suite's own (test_conv2d_fwd_bwd for a1 / a2, the 1e-5 fp32 bound for the heads), scaled by the
magnitude of the fp64 tensor where grey frames make it 255 times larger.

Measured on an MI355X, max |kernel - fp64| / max |torch fp32 on the CPU - fp64| (the run prints them as "ERR" lines):
        [0, 1) frames: a1          a2                heads             grey frames: a1     a2                heads
  S1    5.7e-7 / 5.7e-7   1.6e-7 / 2.4e-7   2.0e-8 / 4.6e-8    1.2e-4 / 1.2e-4   4.4e-5 / 8.2e-5   8.9e-7 / 9.6e-6
  S2    6.7e-7 / 6.7e-7   1.9e-7 / 2.5e-7   4.3e-8 / 5.4e-8    1.0e-4 / 1.0e-4   5.4e-5 / 7.2e-5   1.1e-6 / 5.5e-6
  S3    4.2e-7 / 4.2e-7   1.9e-7 / 3.3e-7   2.0e-8 / 2.2e-8    1.1e-4 / 1.1e-4   3.4e-5 / 6.0e-5   7.5e-7 / 2.1e-6
  S4    5.7e-7 / 5.7e-7   2.1e-7 / 3.0e-7   5.1e-8 / 7.0e-8    1.3e-4 / 1.3e-4   5.7e-5 / 9.2e-5   8.8e-7 / 2.8e-6
  S5    (no stash)        (no stash)        2.0e-8 / 2.7e-8    (no stash)        (no stash)        1.4e-6 / 7.1e-7
  S6    (no stash)        (no stash)        2.1e-8 / 4.5e-8    (no stash)        (no stash)        3.4e-7 / 8.5e-7
  S7    5.1e-7 / 5.1e-7   1.8e-7 / 2.7e-7   1.7e-8 / 2.8e-8    (fp32 frames only)
  S8    4.3e-7 / 4.3e-7   1.6e-7 / 2.7e-7   2.3e-8 / 4.2e-8    1.4e-4 / 1.4e-4   4.2e-5 / 4.7e-5   7.6e-7 / 8.7e-6
(grey a1 / a2 reach about 200 and 140 in magnitude; the heads stay below 1.5 there too, so their bound is 1e-5 in effect.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import a2c_oracle as O  # noqa: E402
from cases import U8FakeEnv, base_hyps, hashf  # noqa: E402
from test_gpu_kernels import close  # noqa: E402
from test_gpu_models import _datas, make_net  # noqa: E402
from test_gpu_ingest import _compare_round, _oracle_rollouts, _pool  # noqa: E402
from test_gpu_small_kernels import MARGIN, draw_uniforms_clear_of_the_cumsum  # noqa: E402
from test_step_shapes import DERIVED, SHAPES  # noqa: E402

DEV = "cuda"
SENT = -77.0
GAMMA = 0.99
torch.set_num_threads(4)
_ERRS = {}          # (shape, frames, array) -> (e_k, e_t): worst over the run, printed at the end


@pytest.fixture(scope="module", autouse=True)
def _print_errors():
    yield
    print("\nmax |kernel - fp64| (e_k) and max |torch fp32 on the CPU - fp64| (e_t) per shape:")
    for k in sorted(_ERRS):
        print("  ERR %-3s %-5s %-5s e_k %.3e e_t %.3e" % (k + _ERRS[k]))


def _u01(shape, seed):
    """uniform in [0, 1) at full fp32 resolution"""
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)).clamp_(max=1 - 2.0 ** -24)


def _grey(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _chain(sd, x, dt):
    """models.py:60-90 on the CPU in dtype dt: a1, a2 (flat (c, y, x)), [logits | value]"""
    g = lambda k: sd[k].to(dt)
    a1 = F.relu(F.conv2d(x.to(dt), g("convs.0.0.weight"), g("convs.0.0.bias"), stride=4))
    a2 = F.relu(F.conv2d(a1, g("convs.1.0.weight"), g("convs.1.0.bias"), stride=2))
    emb = F.linear(a2.flatten(1), g("proj_matrx.weight"), g("proj_matrx.bias"))          # no activation (models.py:73)
    heads = torch.cat([F.linear(emb, g("pi.weight"), g("pi.bias")), F.linear(emb, g("value.weight"), g("value.bias"))], 1)
    return a1.flatten(1), a2.flatten(1), heads


def _push(prev, frame, reset):
    """utils.py:26-43: planes 1..3 of prev (zeros for a reset env), then the new frame.  prev (B, 4, HW), frame (B, HW)"""
    st = torch.cat([prev[:, 1:], frame[:, None]], 1).clone()
    if reset is not None:
        st[reset != 0, :3] = 0
    return st


def _note(sid, frames, name, got, t32, t64):
    e_k = float((got.detach().cpu().double() - t64).abs().max())
    e_t = float((t32.double() - t64).abs().max())
    old = _ERRS.get((sid, frames, name), (0.0, 0.0))
    _ERRS[(sid, frames, name)] = (max(old[0], e_k), max(old[1], e_t))
    print(f"    {sid} {frames} {name}: e_k {e_k:.3e} e_t {e_t:.3e} scale {float(t64.abs().max()):.3g}")


def _check_acts(sid, frames, got, sd, x):
    """a1 | a2 | heads of the kernel against fp64 (e_k and torch-fp32's e_t recorded first); None entries are not compared"""
    r64, r32 = _chain(sd, x, torch.float64), _chain(sd, x, torch.float32)
    for name, g, t32, t64 in zip(("a1", "a2", "heads"), got, r32, r64):
        if g is None:
            continue
        _note(sid, frames, name, g, t32, t64)
    bad = []            # every array is judged before the first failure is raised: a report names all that are off
    for name, g, t64 in zip(("a1", "a2", "heads"), got, r64):
        if g is None:
            continue
        scale = max(1.0, float(t64.abs().max())) if frames == "grey" else 1.0
        if not bool(torch.isfinite(g).all()):       # (a NaN compares false with every bound)
            bad.append(f"{sid} {frames} {name}: not finite")
            continue
        try:
            if name == "heads":
                close(f"{sid} {frames} heads", g, t64, 1e-5 * scale, 1e-5)
            else:
                close(f"{sid} {frames} {name}", g, t64, 2e-6 * max(1.0, float(t64.abs().max())), 1e-5)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, " | ".join(bad)
    return r64, r32


def _record_ref(R, Dn, Dl, VP, v, rew, done, T, t_rec, slot0, pong, boot64=None):
    """a2c_rollout_record (+ a2c_rollout_bootstrap) of include/a2c_mi355x.h in fp32, operation by operation; v = the value the
    previous call left in heads.  -> buffers, and for the bootstrap the rows the freshly computed value enters with their
    fp64 results {e: (reward, delta)}"""
    R, Dn, Dl, VP = R.clone(), Dn.clone(), Dl.clone(), VP.clone()
    g = torch.tensor(GAMMA, dtype=torch.float32)
    fresh = {}
    for b in range(len(rew)):
        e = (slot0 + b) * T + t_rec
        d = 1.0 if (float(done[b]) != 0 or (pong and float(rew[b]) != 0)) else 0.0
        if t_rec > 0:
            Dl[e - 1] = (R[e - 1] + (g * v[b]) * (1 - Dn[e - 1])) - VP[b]
        R[e], Dn[e], VP[b] = rew[b], d, v[b]
        if boot64 is not None:
            if d == 0:
                r64 = float(rew[b]) + float(g) * float(boot64[b])
                fresh[e] = (r64, r64 - float(v[b]))
                R[e], Dn[e], Dl[e] = r64, 1.0, r64 - float(v[b])
            else:
                Dl[e] = R[e] - v[b]
    return R, Dn, Dl, VP, fresh


STEP_CASES = [(s, 3) for s in sorted(SHAPES)] + [("S2", 1), ("S2", 7), ("S4", 1), ("S4", 7)]


@pytest.mark.parametrize("sid,A", STEP_CASES, ids=[f"{s}-A{a}" for s, a in STEP_CASES])
def test_step_kernel_against_fp64(sid, A):
    from a2c_amd import ops
    from a2c_amd._lib import A2CKernelError
    H, W = SHAPES[sid]
    (OH1, OW1), NP1, _, _, Fl, stashable, _, u8able = DERIVED[sid]
    HW, S, B, T = H * W, 4 * H * W, 3, 5
    n1 = 16 * NP1
    ss = (4, H, W)
    net = make_net("A3CModel", ss, A, 256)
    net._ensure_device()
    st = ops.stream()
    net._refresh(st)
    sd = O.formula_state_dict("A3CModel", ss, A, 256)
    hb = net._heads("roll", B)[0]
    assert hb.shape == (B, A + 1)
    seed = 1000 * int(sid[1]) + 10 * A
    PS, OS = S + 4, S + 8                                      # strides of prev and out (floats)
    reset = torch.tensor([0.0, 1.0, 0.0])
    rew = torch.tensor([0.0, 0.0, -1.0])                       # env 1: real done (and reset), env 2: Pong's override
    done = torch.tensor([0.0, 1.0, 0.0])
    hb_prev = torch.from_numpy(hashf(B * (A + 1), seed + 1, -1, 1).reshape(B, A + 1))
    slot0, N = 1, (1 + B) * T

    def bufs():
        R = torch.from_numpy(hashf(N, seed + 2, -1, 1))
        Dn = (torch.from_numpy(hashf(N, seed + 3, 0, 1)) > 0.5).float()
        Dn[(slot0 + 0) * T + 1] = 1.0                          # (the mask (1 - done) of the mid-slot delta: both values occur)
        Dn[(slot0 + 2) * T + 1] = 0.0
        Dl = torch.from_numpy(hashf(N, seed + 4, -1, 1))
        VP = torch.from_numpy(hashf(B, seed + 5, -1, 1))
        return R, Dn, Dl, VP

    last = {}

    def launch(prev, frame=None, frame8=None, fstride=0, with_out=True, stash=False, u=None, t_rec=None, boot=0):
        """one a2c_a3c_step; -> dict of what it left (device tensors, canaried beyond every row)"""
        o = dict(prev=torch.full((B, PS), SENT, device=DEV))
        o["prev"][:, :S] = prev.reshape(B, S).to(DEV)
        kw = dict(prev=o["prev"].data_ptr(), prev_stride=PS)
        if frame is not None:
            o["frame"] = frame.to(DEV).contiguous()
            kw.update(frame_new=o["frame"].data_ptr())
        if frame8 is not None:
            o["frame8"] = frame8.to(DEV).contiguous()
            kw.update(frame_u8=o["frame8"].data_ptr(), frame_stride=fstride)
        if frame is not None or frame8 is not None:
            o["reset"] = reset.to(DEV)
            kw.update(reset_mask=o["reset"].data_ptr())
        if with_out:
            o["out"] = torch.full((B, OS), SENT, device=DEV)
            kw.update(out=o["out"].data_ptr(), out_stride=OS)
        if stash:
            o["a1"] = torch.full((B, n1 + 4), SENT, device=DEV)
            o["a2"] = torch.full((B, Fl + 4), SENT, device=DEV)
            o["ho"] = torch.full((B, A + 3), SENT, device=DEV)
            kw.update(a1_out=o["a1"].data_ptr(), a1_stride=n1 + 4, a2_out=o["a2"].data_ptr(), a2_stride=Fl + 4,
                      heads_out=o["ho"].data_ptr(), heads_out_stride=A + 3)
        if u is not None:
            o["u"] = u.to(DEV)
            o["acts"] = torch.full((B + 1, 3), -7, dtype=torch.int64, device=DEV)
            kw.update(u=o["u"].data_ptr(), actions=o["acts"].data_ptr() + 8, act_stride=3)
        if t_rec is not None:
            o["rew"], o["done"] = rew.to(DEV), done.to(DEV)
            o["R"], o["Dn"], o["Dl"], o["VP"] = (x.to(DEV) for x in bufs())
            kw.update(rew=o["rew"].data_ptr(), done=o["done"].data_ptr(), val_prev=o["VP"].data_ptr(),
                      rewards=o["R"].data_ptr(), dones=o["Dn"].data_ptr(), deltas=o["Dl"].data_ptr(), T=T, t_rec=t_rec,
                      slot0=slot0, gamma=GAMMA, pong=1, bootstrap=boot)
        hb.copy_(hb_prev)
        torch.cuda.synchronize()
        last.clear()
        last.update(o)
        net._step(B, st, **kw)
        torch.cuda.synchronize()
        o["heads"] = hb.clone()
        return o

    def state_ok(o, want):
        """the state row bit for bit, the floats behind it untouched, the input rows unchanged"""
        if "out" in o:
            assert torch.equal(o["out"][:, :S].cpu(), want.reshape(B, S)), "state row"
            assert bool((o["out"][:, S:] == SENT).all()), "floats behind out_stride"
        assert bool((o["prev"][:, S:] == SENT).all())

    def stash_ok(o, frames, x):
        assert bool((o["a1"][:, n1:] == SENT).all()) and bool((o["a2"][:, Fl:] == SENT).all())
        assert bool((o["ho"][:, A + 1:] == SENT).all())
        assert torch.equal(o["ho"][:, :A + 1], o["heads"]), "heads_out is a copy of heads"
        return _check_acts(sid, frames, (o["a1"][:, :n1], o["a2"][:, :Fl], o["heads"]), sd, x)

    def refused(**kw):
        """A2C_ERR_ARG and not a byte written"""
        with pytest.raises(A2CKernelError, match=r"\(code -1\)"):
            launch(**kw)
        torch.cuda.synchronize()
        assert torch.equal(hb.cpu(), hb_prev), "a refused call wrote the heads"
        for k in ("out", "a1", "a2", "ho"):
            assert k not in last or bool((last[k] == SENT).all()), k

    # ------------------------------------------------------------------ fp32 frames
    prev = _u01((B, 4, HW), seed + 6)
    frame = _u01((B, HW), seed + 7)
    want = _push(prev, frame, reset)
    x = want.reshape(B, 4, H, W)
    r64 = _chain(sd, x, torch.float64)
    p64 = F.softmax(r64[2][:, :A], -1)
    u = draw_uniforms_clear_of_the_cumsum(p64, seed + 8)
    want_a = (torch.cumsum(p64, -1) < u.double()[:, None]).sum(1)
    p32 = F.softmax(_chain(sd, x, torch.float32)[2][:, :A], -1)
    assert torch.equal(O.sample_action(p32, u).long(), want_a), "fp32 and fp64 inverse CDF disagree despite the margin"
    assert float((torch.cumsum(p64, -1) - u.double()[:, None]).abs().min()) >= MARGIN

    if not stashable:      # conv1's plane is not a whole number of float4: A2C_ERR_ARG (a2c_a3c_step_args in include/a2c_mi355x.h)
        refused(prev=prev, frame=frame, stash=True)
    # mid-slot record + sampling + stash, state row written
    o = launch(prev, frame=frame, stash=stashable, u=u, t_rec=2)
    state_ok(o, want)
    if stashable:
        stash_ok(o, "f32", x)
    else:
        _check_acts(sid, "f32", (None, None, o["heads"]), sd, x)
    assert torch.equal(o["acts"][:B, 1].cpu(), want_a), f"{int((o['acts'][:B, 1].cpu() != want_a).sum())} actions differ"
    assert bool((o["acts"][:, 0] == -7).all()) and bool((o["acts"][:, 2] == -7).all()) and int(o["acts"][B, 1]) == -7
    R, Dn, Dl, VP, _ = _record_ref(*bufs(), hb_prev[:, A], rew, done, T, 2, slot0, True)
    for name, got, ref in (("rewards", o["R"], R), ("dones", o["Dn"], Dn), ("deltas", o["Dl"], Dl), ("val_prev", o["VP"], VP)):
        assert torch.equal(got.cpu(), ref), name                  # every value read is one a launch left behind: exact
    heads_f32 = o["heads"].clone()
    # last step of the slot + bootstrap, no state row (the other template instance)
    o = launch(prev, frame=frame, with_out=False, u=u, t_rec=T - 1, boot=1)
    state_ok(o, want)
    assert torch.equal(o["heads"], heads_f32), "heads with and without the state row"
    assert torch.equal(o["acts"][:B, 1].cpu(), want_a)
    R, Dn, Dl, VP, fresh = _record_ref(*bufs(), hb_prev[:, A], rew, done, T, T - 1, slot0, True, boot64=r64[2][:, A])
    assert sorted(fresh) == [(slot0 + 0) * T + T - 1], fresh     # env 0 alone is bootstrapped (1: done, 2: Pong's override)
    keep = torch.ones(N, dtype=torch.bool)
    keep[list(fresh)] = False
    assert torch.equal(o["Dn"].cpu(), Dn) and torch.equal(o["VP"].cpu(), VP)
    assert torch.equal(o["R"].cpu()[keep], R[keep]) and torch.equal(o["Dl"].cpu()[keep], Dl[keep])
    for e, (r_, d_) in fresh.items():                             # the value just computed enters: tolerance of the heads
        close("bootstrapped reward", o["R"][e:e + 1], torch.tensor([r_], dtype=torch.float64), 1e-5, 1e-5)
        close("bootstrapped delta", o["Dl"][e:e + 1], torch.tensor([d_], dtype=torch.float64), 1e-5, 1e-5)
    # copy mode: the rows of prev are the state
    o = launch(prev, stash=stashable)
    state_ok(o, prev)
    xc = prev.reshape(B, 4, H, W)
    if stashable:
        stash_ok(o, "f32", xc)
    else:
        _check_acts(sid, "f32", (None, None, o["heads"]), sd, xc)

    # ------------------------------------------------------------------ uint8 frames: grey levels, padded slots
    g_prev = _grey((B, 4, HW), seed + 9).float()
    fstride = -(-HW // 16) * 16 + 48
    g_frame = _grey((B, fstride), seed + 10)
    if not u8able:         # H * W is no multiple of 16: one 16-byte load per thread cannot cover the plane
        refused(prev=g_prev, frame8=g_frame, fstride=fstride)
        _rollout_refused(net, H, W, A)
        return
    want = _push(g_prev, g_frame[:, :HW].float(), reset)
    x = want.reshape(B, 4, H, W)
    o = launch(g_prev, frame8=g_frame, fstride=fstride, stash=stashable, t_rec=2)
    state_ok(o, want)
    if stashable:
        stash_ok(o, "grey", x)
    else:
        _check_acts(sid, "grey", (None, None, o["heads"]), sd, x)
    R, Dn, Dl, VP, _ = _record_ref(*bufs(), hb_prev[:, A], rew, done, T, 2, slot0, True)
    for name, got, ref in (("rewards", o["R"], R), ("dones", o["Dn"], Dn), ("deltas", o["Dl"], Dl), ("val_prev", o["VP"], VP)):
        assert torch.equal(got.cpu(), ref), name
    o2 = launch(g_prev, frame8=g_frame, fstride=fstride, with_out=False)
    assert torch.equal(o2["heads"], o["heads"])


def _rollout_refused(net, H, W, A):
    """a2c_a3c_rollout on a shape without uint8 frames: A2C_ERR_ARG with every pointer valid, nothing written"""
    from a2c_amd import ops
    from a2c_amd._lib import A2CKernelError
    B, T, S = 2, 4, 4 * H * W
    f = lambda *s: torch.full(s, SENT, device=DEV)
    t = dict(states=f(B * T, S), bm=f(B, S), heads=f(B, A + 1), u=f(T, B), vp=f(B), R=f(B * T), Dn=f(B * T), Dl=f(B * T),
             acts=torch.full((B * T,), -7, dtype=torch.int64, device=DEV), cmd=torch.full((B,), -7, dtype=torch.int64, device=DEV),
             rec=torch.full((B,), -7, dtype=torch.int64, device=DEV), err=torch.full((1,), -7, dtype=torch.int32, device=DEV),
             frames=torch.full((B, H * W + 12), 7, dtype=torch.uint8, device=DEV))
    before = {k: v.clone() for k, v in t.items()}
    P = net.P
    with pytest.raises(A2CKernelError, match=r"\(code -1\)"):
        ops.a3c_rollout(ops.stream(), B=B, C=4, H=H, W=W, n_actions=A, states=t["states"].data_ptr(), bookmark=t["bm"].data_ptr(),
                        wfrag1=net._c1.wf.data_ptr(), bias1=P("convs.0.0.bias").data_ptr(), wfrag2=net._c2.wf.data_ptr(),
                        bias2=P("convs.1.0.bias").data_ptr(), Wc=net._Wc.data_ptr(), bc=net._bc.data_ptr(),
                        heads=t["heads"].data_ptr(), ldh=A + 1, u=t["u"].data_ptr(), u_stride=B, actions=t["acts"].data_ptr(),
                        val_prev=t["vp"].data_ptr(), rewards=t["R"].data_ptr(), dones=t["Dn"].data_ptr(),
                        deltas=t["Dl"].data_ptr(), T=T, slot0=0, gamma=GAMMA, pong=1, cmd=t["cmd"].data_ptr(),
                        rec=t["rec"].data_ptr(), frames=t["frames"].data_ptr(), frame_stride=H * W + 12, frame_bits=0,
                        conv1_weight=P("convs.0.0.weight").data_ptr(), seq0=0, env0=0, err=t["err"].data_ptr(), timeout_ticks=1)
    torch.cuda.synchronize()
    for k in t:
        assert torch.equal(t[k], before[k]), k


# ====================================================================================== rollouts through the Runner
def _stash_against_fp64(sid, net, D, A, N):
    """what the rollout left in the update's buffers for every state of the rollout buffer, against fp64"""
    H, W = SHAPES[sid]
    sd = O.formula_state_dict("A3CModel", (4, H, W), A, 256)
    ws = net.ws("train")
    a1 = ws.get("a1", (N,) + net._c1.out_shape).reshape(N, -1)
    a2 = ws.get("a2", (N,) + net._c2.out_shape).reshape(N, -1)
    _check_acts(sid, "01", (a1, a2, net._heads("train", N)[0]), sd, D["states"].cpu())


def _rollouts(sid, A, monkeypatch, no_ring=False, bits=False, lazy=False):
    from a2c_amd import ops
    from a2c_amd.runner import Runner
    if no_ring:
        monkeypatch.setenv("A2C_NO_RING", "1")
    H, W = SHAPES[sid]
    stashable, lanemaskable = DERIVED[sid][5], DERIVED[sid][6]
    B, T, ss = 3, 5, (4, H, W)
    ekws = [dict(env_id=j, frame_shape=(1, H, W), rew_period=3 + j % 3, done_period=4 + 2 * j) for j in range(B)]
    hyps = base_hyps(env_type="FakePong-v0", n_tsteps=T, n_rollouts=B, action_shift=0, n_envs=B, env_timeout_s=20.0,
                     **(dict(frame_store=True, lazy_states=True) if lazy else {}))
    net = make_net("A3CModel", ss, A, 256)
    onet = O.OracleNet("A3CModel", ss, A, 256)
    D = _datas(B * T, ss, False, actions_on_host=False)
    us = torch.from_numpy(hashf(2 * T * B, 901 + H + W + A, 0, 1).reshape(2, T, B))
    usd = us.to(DEV)
    rnd = [0]
    pool = _pool(U8FakeEnv, ekws, 2, pong=True, **(dict(frame_bits=True) if bits else {}))
    r = Runner(D, hyps, None, None, None, env_pool=pool, ingest="zero-copy",
               uniform_fn=lambda t, Bn, env0: usd[rnd[0], t, env0:env0 + Bn].contiguous())
    try:
        refs = _oracle_rollouts("A3CModel", onet, hyps, ekws, us, 2, B, T, ss)
        for rnd[0] in range(2):
            r.rollout(net, list(range(B)), hyps)
            r.finish()
            if lazy:
                assert net._stash_frames is not None and r._states_stale
                if rnd[0] == 0:
                    assert float(D["states"].abs().sum()) == 0.0          # never written by the rollout ...
                r.materialize_states()                                     # ... a2c_frames_to_states expands the store
            _compare_round(D, refs[rnd[0]], False)
            assert (net._stash is not None) == stashable
            if stashable:
                _stash_against_fp64(sid, net, D, A, B * T)
        assert pool.frame_dtype == np.uint8 and pool.seq == 2 * T and r._zero_copy_ok(net)
        if bits:
            assert pool.transport == "bits" and pool.header.frame_bytes == H * W // 8 and r.bits
        assert ops.a3c_ring_supported(B, 4, H, W, A, net.P("convs.0.0.weight").data_ptr()) == (not no_ring)
        if not lanemaskable:      # the update masks conv2's backward-data with the float rows
            assert net._a1_lanemask_rows(B * T) is None and not net._stash_lm
        if not stashable:         # no stash is handed out: the update recomputes the activations
            assert net.stash_rows(D["states"], B * T, T=T) is None
    finally:
        r.close()


ROLL_CASES = [("S2", 3), ("S3", 4), ("S4", 7), ("S5", 3), ("S8", 4)]


@pytest.mark.parametrize("body", ["ring", "per_step"])
@pytest.mark.parametrize("sid,A", ROLL_CASES, ids=[f"{s}-A{a}" for s, a in ROLL_CASES])
def test_rollouts_match_oracle(sid, A, body, monkeypatch):
    """two consecutive rounds of B slots over a process pool of uint8 envs, ring kernel and per-step persistent body"""
    _rollouts(sid, A, monkeypatch, no_ring=(body == "per_step"))


@pytest.mark.parametrize("lazy", [False, True], ids=["packed", "packed_frame_store_lazy_states"])
@pytest.mark.parametrize("sid,A", [("S2", 4), ("S4", 3)], ids=["S2-A4", "S4-A3"])
def test_rollouts_on_the_packed_transport_match_oracle(sid, A, lazy, monkeypatch):
    """one bit per pixel through the ring kernel; with the single-frame store and lazy states the fp32 rows come from
    a2c_frames_to_states"""
    _rollouts(sid, A, monkeypatch, bits=True, lazy=lazy)


# ====================================================================================== rollout -> update -> rollout
def _make_run(sid, A, hyps, usd, rnd):
    from a2c_amd.runner import Runner
    H, W = SHAPES[sid]
    B, T = hyps["n_envs"], hyps["n_tsteps"]
    ekws = [dict(env_id=j, frame_shape=(1, H, W), rew_period=2 + j % 2, done_period=4 + j) for j in range(B)]
    net = make_net("A3CModel", (4, H, W), A, 256)
    D = _datas(B * T, (4, H, W), False, actions_on_host=False)
    pool = _pool(U8FakeEnv, ekws, 2, pong=True)
    fn = None if usd is None else (lambda t, Bn, env0: usd[rnd[0], t, env0:env0 + Bn].contiguous())
    return net, D, ekws, Runner(D, hyps, None, None, None, env_pool=pool, ingest="zero-copy", uniform_fn=fn)


@pytest.mark.parametrize("sid", ["S2", "S3", "S6"])
def test_rollout_update_rollout_matches_oracle(sid):
    """three rounds with update_model in between, as tests/test_gpu_ingest.py runs them at 84 x 84 (same tolerances): S2
    reads the stash, S3 reads it with float masks, S6 has none and recomputes"""
    from a2c_amd.updater import Updater
    H, W = SHAPES[sid]
    B, T, A, ss = 3, 5, 3, (4, H, W)
    hyps = base_hyps(env_type="FakePong-v0", n_tsteps=T, n_rollouts=B, action_shift=0, n_envs=B, lr=1e-2,
                     optim_type="RMSprop", use_bptt=False, h_size=256)
    us = torch.from_numpy(hashf(3 * T * B, 977 + H, 0, 1).reshape(3, T, B))
    rnd = [0]
    net, D, ekws, r = _make_run(sid, A, hyps, us.to(DEV), rnd)
    onet = O.OracleNet("A3CModel", ss, A, 256)
    upd = Updater(net, hyps)
    try:
        refs = _oracle_rollouts("A3CModel", onet, hyps, ekws, us, 3, B, T, ss, updater=O.OracleUpdater(onet, hyps))
        for rnd[0] in range(3):
            r.rollout(net, list(range(B)), hyps)
            r.finish()
            assert (net._stash is not None) == DERIVED[sid][5]
            if sid == "S3":
                assert not net._stash_lm
            tol = 1e-5 if rnd[0] == 0 else 2e-3
            assert torch.equal(D["states"].cpu(), refs[rnd[0]]["states"])
            assert torch.equal(D["dones"].cpu(), refs[rnd[0]]["dones"])
            close("deltas", D["deltas"], refs[rnd[0]]["deltas"], tol, tol)
            mism = (D["actions"].cpu() != refs[rnd[0]]["actions"]).sum().item()
            assert mism == 0 if rnd[0] == 0 else mism <= 1, mism
            if rnd[0] < 2:
                info = upd.update_model(D)
                oi = refs[rnd[0]]["info"]
                for k in oi:
                    assert abs(info[k] - oi[k]) <= 1e-4 + 2e-3 * abs(oi[k]), (rnd[0], k, info[k], oi[k])
        assert not torch.allclose(D["deltas"].cpu(), _oracle_rollouts("A3CModel", O.OracleNet("A3CModel", ss, A, 256), hyps, ekws,
                                                                      us, 3, B, T, ss)[2]["deltas"], atol=1e-3)
    finally:
        r.close()


@pytest.mark.parametrize("sid", ["S2", "S3"])
def test_update_from_the_stash_equals_the_recomputed_one(sid, monkeypatch):
    """tests/test_gpu_ingest.py's check of the activation stash at 84 x 84, with its tolerances"""
    from a2c_amd.updater import Updater
    B, T, A = 3, 5, 3
    hyps = base_hyps(env_type="FakePong-v0", n_tsteps=T, n_rollouts=B, action_shift=0, n_envs=B, lr=1e-3, use_bptt=False)
    res = {}
    for stash in (True, False):
        if not stash:
            monkeypatch.setenv("A2C_NO_STASH", "1")
        net, D, _, r = _make_run(sid, A, hyps, None, None)
        torch.manual_seed(5)
        try:
            r.rollout(net, list(range(B)), hyps)
            r.finish()
            assert (net._stash is not None) == stash
            info = Updater(net, hyps).update_model(D)
            assert net._stash is None
            res[stash] = (info, net._arena.train_grads().cpu().clone(), {k: v.cpu().clone() for k, v in D.items()})
        finally:
            r.close()
    for k in ("states", "actions", "rewards", "deltas"):
        assert torch.equal(res[True][2][k], res[False][2][k]), k
    for k in res[True][0]:
        assert res[True][0][k] == pytest.approx(res[False][0][k], rel=2e-6, abs=1e-8), k
    ga, gb = res[True][1], res[False][1]
    close("gradient arena", ga, gb, 2e-6 * float(gb.abs().max()), 1e-5)


def test_lazy_states_without_a_stash_are_materialised_for_the_update():
    """S5 on the single-frame store with lazy states: no stash is handed out, so the ring kernel leaves neither fp32 state
    rows nor activations, and update_model has to expand the rows from the store itself (A3CModel._need_states) before it
    recomputes the forward.  Rollout, update, rollout against the oracle, tolerances of the test above."""
    from a2c_amd.updater import Updater
    sid = "S5"
    H, W = SHAPES[sid]
    B, T, A, ss = 3, 5, 3, (4, H, W)
    hyps = base_hyps(env_type="FakePong-v0", n_tsteps=T, n_rollouts=B, action_shift=0, n_envs=B, lr=1e-2,
                     optim_type="RMSprop", use_bptt=False, h_size=256, frame_store=True, lazy_states=True)
    us = torch.from_numpy(hashf(2 * T * B, 991, 0, 1).reshape(2, T, B))
    rnd = [0]
    net, D, ekws, r = _make_run(sid, A, hyps, us.to(DEV), rnd)
    onet = O.OracleNet("A3CModel", ss, A, 256)
    upd = Updater(net, hyps)
    try:
        refs = _oracle_rollouts("A3CModel", onet, hyps, ekws, us, 2, B, T, ss, updater=O.OracleUpdater(onet, hyps))
        for rnd[0] in range(2):
            r.rollout(net, list(range(B)), hyps)
            r.finish()
            assert net._stash is None and net._stash_frames is None and r._states_stale
            if rnd[0] == 0:
                assert float(D["states"].abs().sum()) == 0.0          # the rollout wrote no fp32 row
                info = upd.update_model(D)
                assert not r._states_stale                             # the update asked for the rows
                for k, v in refs[0]["info"].items():
                    assert abs(info[k] - v) <= 1e-4 + 2e-3 * abs(v), (k, info[k], v)
            else:
                r.materialize_states()
            tol = 1e-5 if rnd[0] == 0 else 2e-3
            assert torch.equal(D["states"].cpu(), refs[rnd[0]]["states"])
            assert torch.equal(D["dones"].cpu(), refs[rnd[0]]["dones"])
            close("deltas", D["deltas"], refs[rnd[0]]["deltas"], tol, tol)
            mism = (D["actions"].cpu() != refs[rnd[0]]["actions"]).sum().item()
            assert mism == 0 if rnd[0] == 0 else mism <= 1, mism
    finally:
        r.close()


@pytest.mark.parametrize("sid", sorted(SHAPES))
def test_conv2_fragments_arrive_in_the_order_the_step_kernels_assume(sid):
    """a2c_conv2d_prep_weights(kind 0) lays conv2's 64 steps as (c4, ky, kx) where conv.hip's row-run kernel takes the layer
    and tap-major (tap * 4 + c4) elsewhere; step.hip restates that choice as "conv1's output width is a multiple of 4"
    (StepP::w2_tap_major) and un-permutes on load.  The two must not drift apart: the prepared buffer, element by element"""
    from a2c_amd import ops
    H, W = SHAPES[sid]
    (OH1, OW1) = DERIVED[sid][0]
    net = make_net("A3CModel", (4, H, W), 3, 256)
    net._ensure_device()
    net._refresh(ops.stream())
    torch.cuda.synchronize()
    w2 = O.formula_state_dict("A3CModel", (4, H, W), 3, 256)["convs.1.0.weight"]          # (32, 16, 4, 4)
    assert (net._c2.d.H, net._c2.d.W) == (OH1, OW1)
    want = torch.empty(64, 2, 64)
    lane = torch.arange(64)
    for c4 in range(4):
        for ky in range(4):
            for kx in range(4):
                step = (ky * 4 + kx) * 4 + c4 if OW1 % 4 else (c4 * 4 + ky) * 4 + kx
                for mt in range(2):
                    want[step, mt] = w2[mt * 16 + (lane & 15), 4 * c4 + (lane >> 4), ky, kx]
    assert torch.equal(net._c2.wf[:64 * 2 * 64].cpu(), want.reshape(-1))
