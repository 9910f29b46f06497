"""-m gpu: a2c_vecnorm_step (csrc/vecnorm.hip) against its host twin ``a2c_amd.vecnorm.RunningNorm``: the state block bit for
bit (fp64 +, -, x, / in a fixed order), the fp32 outputs bit for bit (fp64 square root and division, one rounding to fp32),
everything not addressed untouched, every A2C_ERR_ARG case without a launch."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GAMMA = 0.99
STEPS = 6
T, SLOT0, ENV0, PAD_ENVS, PAD_STRIDE = 7, 2, 5, 9, 3
MODES = ("obs", "rew", "both", "frozen")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _same(got, want, what):
    """bit equality of two arrays, the mismatches printed before the assertion"""
    got, want = np.asarray(got), np.asarray(want)
    bad = _bits(got) != _bits(want)
    if bad.any():
        i = np.argwhere(bad)[0]
        print(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {tuple(i)}: got {got[tuple(i)]!r}, want {want[tuple(i)]!r}; "
              f"max ulp {int(np.abs(_bits(got).astype(np.int64) - _bits(want).astype(np.int64)).max())}")
    assert not bad.any(), what


def _inputs(B, L, C, seed):
    """STEPS env steps of B envs: next-state rows with padded strides (every plane random: the older ones must come back
    untouched), reward rows of very different sizes, dones in about a third of the places; feature L - 1 is a constant"""
    g = np.random.default_rng(seed)
    stride = C * L + PAD_STRIDE
    scale = (10.0 ** g.uniform(-2, 2, L)).astype(np.float32)
    shift = g.uniform(-5, 5, L).astype(np.float32)
    rows = g.standard_normal((STEPS, B, stride)).astype(np.float32)
    new = rows[:, :, (C - 1) * L:C * L]
    new *= scale
    new += shift
    new[:, :, L - 1] = 0.0 if L == 4 else 1.0
    N = (SLOT0 + B + 1) * T
    rew = (g.standard_normal((STEPS, N)) * 10.0 ** g.uniform(-1, 2, (STEPS, 1))).astype(np.float32)
    done = (g.uniform(size=(STEPS, N)) < 0.3).astype(np.float32)
    done[2] = 1.0                              # ... and one step that closes every env, so that B = 1 sees a done too
    return rows, rew, done


def _play(B, L, C, mode):
    from a2c_amd.vecnorm import DeviceVecNorm, RunningNorm
    rows, rew, done = _inputs(B, L, C, 1000 * B + 10 * L + C)
    B_pool = ENV0 + B + PAD_ENVS
    kw = dict(eps=1e-8, clip_obs=3.0, clip_rew=2.5)
    dv, tw = DeviceVecNorm(L, B_pool, GAMMA, device=DEV, **kw), RunningNorm(L, B_pool, GAMMA, **kw)
    _same(dv.block.cpu().numpy(), tw.to_block(), "the initial block")
    assert dv.block.numel() == 4 + 2 * L + B_pool and tw.to_block()[0] == 1e-4
    if mode == "frozen":       # moments worth freezing first
        tw.ret[:] = np.arange(B_pool) * 0.5
        tw.step(rows[0][:, (C - 1) * L:C * L], rew[0][:B], done[0][:B], ENV0)
        dv.load(tw)
    stride = rows.shape[2]
    clipped = zeroed = 0
    for k in range(STEPS):
        t = k % T
        d_rows = torch.from_numpy(rows[k]).to(DEV)
        d_rew, d_done = torch.from_numpy(rew[k]).to(DEV), torch.from_numpy(done[k]).to(DEV)
        idx = (SLOT0 + np.arange(B)) * T + t
        x = rows[k][:, (C - 1) * L:C * L]
        before = tw.to_block()
        want_o, want_r = tw.step(x if mode != "rew" else None, rew[k][idx] if mode in ("rew", "both") else None,
                                 done[k][idx] if mode in ("rew", "both") else None, ENV0, update=mode != "frozen")
        dv.launch(B, ENV0, out_ptr=d_rows.data_ptr() if mode != "rew" else 0, out_stride=stride, C=C,
                  rewards=d_rew if mode in ("rew", "both") else None, dones=d_done if mode in ("rew", "both") else None,
                  T=T, t=t, slot0=SLOT0, update=mode != "frozen")
        _same(dv.block.cpu().numpy(), tw.to_block(), f"block after step {k}")
        if mode == "frozen":
            _same(tw.to_block(), before, "the twin's block in frozen mode")
        exp_rows, exp_rew = rows[k].copy(), rew[k].copy()
        if want_o is not None:
            exp_rows[:, (C - 1) * L:C * L] = want_o
            clipped += int((np.abs(want_o) == 3.0).sum())
        if want_r is not None:
            exp_rew[idx] = want_r
            clipped += int((np.abs(want_r) == 2.5).sum())
            zeroed += int((done[k][idx] != 0).sum())
        _same(d_rows.cpu().numpy(), exp_rows, f"next-state rows after step {k}")
        _same(d_rew.cpu().numpy(), exp_rew, f"reward rows after step {k}")
        _same(d_done.cpu().numpy(), done[k], "dones")
    blk = tw.to_block()
    ret = blk[4 + 2 * L:]
    count = np.float64(1e-4)
    for _ in range(STEPS):
        count = count + np.float64(B)
    if mode in ("rew", "both"):
        assert zeroed > 0 and (ret[:ENV0] == 0).all() and (ret[ENV0 + B:] == 0).all() and blk[1 + 2 * L] == count
    if mode in ("obs", "both"):
        assert blk[0] == count and blk[1 + 2 * L] == (1e-4 if mode == "obs" else blk[0])
    if mode == "frozen":
        assert (ret[:ENV0] == np.arange(ENV0) * 0.5).all(), "ret outside the range"
    return clipped


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("L", [4, 8])
@pytest.mark.parametrize("B", [1, 3, 64, 257, 1000])
def test_kernel_equals_the_twin(B, L, C):
    """below one wave, one wave, past one pass of the 256 lanes, several passes; env0 = 5 inside a larger pool; six steps with
    dones; observations only, rewards only, both, frozen"""
    clipped = {mode: _play(B, L, C, mode) for mode in MODES}
    print(f"vecnorm B={B} L={L} C={C}: values at a clip {clipped}")
    if B >= 64:
        assert clipped["both"] > 0


def test_more_features_than_one_chunk():
    """L = 19 and L = 64: the tree runs over chunks of 8 features, the last one partial"""
    for L in (19, 64):
        _play(70, L, 2, "both")


def test_argument_checks_return_err_arg_without_launching():
    from a2c_amd import _lib
    from a2c_amd.vecnorm import DeviceVecNorm
    lib = _lib.load()
    B, L, C, B_pool = 3, 4, 2, 8
    dv = DeviceVecNorm(L, B_pool, GAMMA, device=DEV)
    block0 = dv.block.clone()
    f32 = dict(dtype=torch.float32, device=DEV)
    bufs = {n: torch.full((256,), -3.0, **f32) for n in ("out", "rewards", "dones")}
    ptr = {n: x.data_ptr() + 64 for n, x in bufs.items()}

    def step(block=dv.block.data_ptr(), **o):
        a = dict(B=B, env0=1, B_pool=B_pool, L=L, C=C, update=1, out=ptr["out"], out_stride=C * L, rewards=ptr["rewards"],
                 dones=ptr["dones"], T=4, t=1, slot0=0, gamma=GAMMA, eps=1e-8, clip_obs=10.0, clip_rew=10.0)
        a.update(o)
        return lib.a2c_vecnorm_step(block, ctypes.byref(_lib.VecNormArgs(**a)), None)
    bad = [dict(block=None), dict(B=0), dict(B=-1), dict(L=0), dict(L=65), dict(env0=-1), dict(env0=6), dict(B=8),
           dict(B_pool=0), dict(t=-1), dict(t=4), dict(T=0), dict(slot0=-1), dict(out_stride=C * L - 1), dict(out_stride=0),
           dict(C=0), dict(eps=0.0), dict(eps=-1e-8), dict(clip_obs=0.0), dict(clip_rew=0.0), dict(clip_obs=-1.0),
           dict(clip_rew=-2.0), dict(out=None, rewards=None), dict(dones=None), dict(update=0),
           dict(eps=float("nan"))]
    for o in bad:
        assert step(**o) == -1, o
    assert lib.a2c_vecnorm_step(dv.block.data_ptr(), None, None) == -1
    assert lib.a2c_vecnorm_init(None, L, B_pool, None) == -1 and lib.a2c_vecnorm_init(dv.block.data_ptr(), 0, B_pool, None) == -1
    assert lib.a2c_vecnorm_init(dv.block.data_ptr(), 65, B_pool, None) == -1
    assert lib.a2c_vecnorm_init(dv.block.data_ptr(), L, 0, None) == -1
    assert lib.a2c_vecnorm_state_bytes(L, B_pool) == 8 * (4 + 2 * L + B_pool)
    assert lib.a2c_vecnorm_state_bytes(0, 4) == 0 and lib.a2c_vecnorm_state_bytes(65, 4) == 0
    assert lib.a2c_vecnorm_state_bytes(4, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(dv.block, block0)
    for n, x in bufs.items():
        assert bool((x == -3).all()), n               # nothing ran
    # ... and the valid calls are accepted: both parts, either one, frozen observations, a padded stride
    assert step() == 0 and step(out=None) == 0 and step(rewards=None, dones=None) == 0
    assert step(rewards=None, update=0) == 0 and step(out_stride=C * L + 5) == 0
    torch.cuda.synchronize()
    assert not torch.equal(dv.block, block0)
    assert bool((bufs["out"][:16] == -3).all()) and bool((bufs["rewards"][:16] == -3).all())
    assert bool((bufs["dones"] == -3).all())


def test_device_step_has_the_twins_surface():
    """``DeviceVecNorm.step`` on (B, L) / (B,) tensors in place, ``snapshot`` / ``load`` / ``state_dict``"""
    from a2c_amd.vecnorm import DeviceVecNorm, RunningNorm
    B, L = 37, 4
    g = np.random.default_rng(3)
    dv, tw = DeviceVecNorm(L, B, GAMMA, device=DEV), RunningNorm(L, B, GAMMA)
    for k in range(3):
        o, r = g.standard_normal((B, L)).astype(np.float32) * 4, g.standard_normal(B).astype(np.float32) * 30
        d = (g.uniform(size=B) < 0.2).astype(np.float32)
        wo, wr = tw.step(o, r, d, 0)
        go, gr = dv.step(torch.from_numpy(o).to(DEV), torch.from_numpy(r).to(DEV), torch.from_numpy(d).to(DEV), 0)
        _same(go.cpu().numpy(), wo, "obs"); _same(gr.cpu().numpy(), wr, "rewards")
    snap = dv.snapshot()
    _same(snap.to_block(), tw.to_block(), "snapshot")
    other = DeviceVecNorm(L, B, 0.5, clip_obs=1.0, device=DEV).load_state_dict(dv.state_dict())
    assert torch.equal(other.block, dv.block) and other.gamma == GAMMA and other.clip_obs == 10.0
    with pytest.raises(ValueError):
        DeviceVecNorm(L, B + 1, GAMMA, device=DEV).load(snap)
