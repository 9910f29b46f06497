"""The clipped multi-epoch update (hyps["ppo_epochs"] / hyps["ppo_clip"]) without a GPU: the two
entry points are declared, exported and refuse their bad arguments before touching the device; ``ops.ppo_rows_host`` (the
row rule the kernels and the docs point at) against float64 autograd of the textbook expression; the defaults and the
refusals of ``train()``.  The kernels and the update themselves: tests/test_gpu_ppo.py."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("a2c_ppo_loss_fwd_bwd", "a2c_gauss_ppo_fwd_bwd")
ERR_ARG = -1


def test_header_declares_and_library_exports_both_entry_points():
    from a2c_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "a2c_mi355x.h")).read()
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared in include/a2c_mi355x.h"
        params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
        assert len(params) == len(_lib.SIGNATURES[name][1]), (name, params)
        for want in ("float clip", "int record", "double *logp_old", "double *loss_sums", "double *reduce_scratch",
                     "a2c_stream_t stream"):
            assert want in params, (name, want)
        assert params.index("float clip") == params.index("float entr_coef") + 1      # the sibling's arguments up to entr_coef
        assert callable(getattr(lib, name))


# ---------------------------------------------------------------------------------------------------- arguments
P = 4096        # any non-NULL address: a refused call reads none of them
DISCRETE = dict(logits=P, ld_logits=6, vals=P, val_stride=1, actions=P, advs=P, returns=P, adv_sums=None, n_local=4,
                n_global=4, A=6, pi_coef=1.0, val_coef=0.5, entr_coef=0.01, clip=0.2, record=0, logp_old=P, dlogits=P, ldd=6,
                dvals=P, dval_stride=1, loss_sums=P, reduce_scratch=P)
GAUSS = dict(heads=P, ld_heads=7, vals=P, val_stride=7, actions=P, ld_act=3, advs=P, returns=P, adv_sums=None, n_local=4,
             n_global=4, n=3, pi_coef=1.0, val_coef=0.5, entr_coef=0.01, clip=0.2, record=1, logp_old=P, dheads=P, ldd=7,
             dvals=P, dval_stride=7, loss_sums=P, reduce_scratch=P)
NEW_BAD = [dict(clip=0.0), dict(clip=-0.2), dict(clip=float("inf")), dict(clip=float("nan")), dict(record=2), dict(record=-1),
           dict(logp_old=None)]
COMMON_BAD = [dict(n_local=-1), dict(n_global=3), dict(loss_sums=None), dict(reduce_scratch=None),
              dict(adv_sums=P, n_local=1, n_global=1), dict(vals=None), dict(advs=None), dict(returns=None), dict(actions=None),
              dict(dvals=None)]
DISCRETE_BAD = [dict(A=0), dict(A=33), dict(logits=None), dict(dlogits=None)]
GAUSS_BAD = [dict(n=0), dict(n=65), dict(ld_heads=5), dict(ld_act=2), dict(ldd=5), dict(heads=None), dict(dheads=None),
             dict(n_local=0, n_global=0)]


@pytest.mark.parametrize("name,good,bad", [(NAMES[0], DISCRETE, DISCRETE_BAD), (NAMES[1], GAUSS, GAUSS_BAD)])
def test_bad_arguments_return_err_arg_without_launching(name, good, bad):
    """everything the sibling entry point rejects, and clip / record / logp_old: refused before anything touches the device"""
    from a2c_amd import _lib
    fn = getattr(_lib.load(), name)
    order = list(good)
    assert len(_lib.SIGNATURES[name][1]) == len(order) + 1
    for o in NEW_BAD + COMMON_BAD + bad:
        a = dict(good, **o)
        assert fn(*[a[k] for k in order], None) == ERR_ARG, (name, o)
        # a bad clip / record / logp_old is refused for an empty share too (n_local == 0 would otherwise return OK)
        if o in NEW_BAD:
            a = dict(a, n_local=0)
            assert fn(*[a[k] for k in order], None) == ERR_ARG, (name, o, "n_local = 0")


# ---------------------------------------------------------------------------------------------------- the row rule
@pytest.mark.parametrize("clip", [0.2, 0.02, 0.5])
def test_ppo_rows_host_is_the_clipped_surrogate_and_keep_its_derivative(clip):
    """against float64 autograd of min(r w, clamp(r, 1 - c, 1 + c) w) on rows whose ratio stays 1e-3 away from the edges: the
    values (the rule takes clip as the float32 the kernels receive: 1 +- clip moves by at most 2^-25 = 3e-8, relative), and
    keep == (d surr / d logp != 0) wherever w != 0"""
    from a2c_amd import ops
    g = torch.Generator().manual_seed(7)
    N = 4000
    logp_old = torch.randn(N, generator=g, dtype=torch.float64) * 3 - 2
    d = (torch.rand(N, generator=g, dtype=torch.float64) * 2 - 1) * 3 * clip
    d[::97] = 0.0
    w = torch.randn(N, generator=g, dtype=torch.float64)
    w[::50] = 0.0
    r0 = d.exp()
    ok = ((r0 - (1 + clip)).abs() > 1e-3) & ((r0 - (1 - clip)).abs() > 1e-3)
    logp_old, d, w = logp_old[ok], d[ok], w[ok]
    assert int(ok.sum()) > N // 2
    logp = (logp_old + d).clone().requires_grad_(True)
    r_t = (logp - logp_old).exp()
    surr_t = torch.minimum(r_t * w, torch.clamp(r_t, 1 - clip, 1 + clip) * w)
    surr_t.sum().backward()
    r, surr, keep = ops.ppo_rows_host(logp.detach().numpy(), logp_old.numpy(), w.numpy(), clip)
    assert r.dtype == np.float64 and surr.dtype == np.float64 and keep.dtype == np.bool_
    np.testing.assert_allclose(r, r_t.detach().numpy(), rtol=1e-15, atol=0)
    np.testing.assert_allclose(surr, surr_t.detach().numpy(), rtol=1e-7, atol=0)
    nz = (w != 0).numpy()
    moved = (logp.grad != 0).numpy()
    assert np.array_equal(keep[nz], moved[nz])
    assert keep[~nz].all()                      # a row of weight zero is never counted as clipped
    # all five situations occur: inside, and (sign of w) x (side of the range) outside
    wn, hi, lo = w.numpy(), r > 1 + clip, r < 1 - clip
    for sel, kept in ((~hi & ~lo & nz, True), ((wn > 0) & hi, False), ((wn < 0) & lo, False), ((wn > 0) & lo, True),
                      ((wn < 0) & hi, True)):
        assert sel.any() and (keep[sel] == kept).all()
    # an overflowed ratio on a clipped row: r = inf, the surrogate the clipped branch, keep False
    r, surr, keep = ops.ppo_rows_host([0.0], [-800.0], [2.0], clip)
    assert np.isinf(r[0]) and not keep[0] and surr[0] == (1.0 + float(np.float32(clip))) * 2.0


# ---------------------------------------------------------------------------------------------------- train()
def test_defaults():
    from a2c_amd import training
    assert training.DEFAULTS["ppo_epochs"] == 1 and training.DEFAULTS["ppo_clip"] == 0.2
    assert isinstance(training.DEFAULTS["ppo_epochs"], int)


def _hyps(**kw):
    return dict(dict(exp_name="e", main_path="unused", model="FCModel", env_type="Pendulum-device", n_envs=2, n_tsteps=2, seed=1,
                     gauss_loss="exact"), **kw)


REFUSALS = [  # hyps, the key the message names
    (dict(ppo_epochs=0), "ppo_epochs"), (dict(ppo_epochs=-3), "ppo_epochs"), (dict(ppo_epochs=2.0), "ppo_epochs"),
    (dict(ppo_epochs="2"), "ppo_epochs"), (dict(ppo_epochs=True), "ppo_epochs"), (dict(ppo_epochs=None), "ppo_epochs"),
    (dict(ppo_clip=0.0), "ppo_clip"), (dict(ppo_clip=-0.1), "ppo_clip"), (dict(ppo_clip=float("nan")), "ppo_clip"),
    (dict(ppo_clip=float("inf")), "ppo_clip"), (dict(ppo_clip="0.2"), "ppo_clip"), (dict(ppo_clip=None), "ppo_clip"),
    (dict(ppo_epochs=1, ppo_clip=0.0), "ppo_clip"),                  # a bad value is refused whether or not it would be used
    (dict(ppo_epochs=2, model="A3CModel", env_type="Pong-device", gauss_loss="reference"), "ppo_epochs"),
    (dict(ppo_epochs=2, model="GRUModel", env_type="Pong-device", gauss_loss="reference"), "ppo_epochs"),
    (dict(ppo_epochs=2, model="ConvModel", env_type="Breakout-device", gauss_loss="reference"), "ppo_epochs"),
    (dict(ppo_epochs=3, gauss_loss="reference"), "ppo_epochs"),      # a continuous family under the reference's Gaussian loss
    (dict(ppo_epochs=3, env_type="Point-device", model="GRUFCModel", gauss_loss="reference"), "ppo_epochs"),
]


@pytest.mark.parametrize("kw,key", REFUSALS, ids=[f"{i}-{k}" for i, (_, k) in enumerate(REFUSALS)])
def test_complete_hyps_refuses_naming_the_key(kw, key, tmp_path):
    from a2c_amd import training
    with pytest.raises(ValueError, match=key):
        training._complete_hyps(_hyps(**kw), None, None)
    with pytest.raises(ValueError, match=key):          # and train() before anything is written
        training.train(None, _hyps(main_path=str(tmp_path), **kw), verbose=False)
    assert not list(tmp_path.iterdir())


def test_complete_hyps_accepts_what_the_update_covers():
    from a2c_amd import training
    for kw in (dict(), dict(ppo_epochs=1, gauss_loss="reference"), dict(ppo_epochs=4, ppo_clip=0.1),
               dict(ppo_epochs=2, ppo_clip=1, model="GRUFCModel"),
               dict(ppo_epochs=2, env_type="CartPole-device", gauss_loss="reference"),        # discrete actions
               dict(ppo_epochs=1, model="A3CModel", env_type="Pong-device", gauss_loss="reference")):
        hyps = training._complete_hyps(_hyps(**kw), None, None)[0]
        assert hyps["ppo_epochs"] == kw.get("ppo_epochs", 1) and hyps["ppo_clip"] == kw.get("ppo_clip", 0.2)
    # an env_fn tells its action kind through hyps["is_discrete"]
    with pytest.raises(ValueError, match="ppo_epochs"):
        training._complete_hyps(_hyps(ppo_epochs=2, gauss_loss="reference", is_discrete=False, action_size=2), lambda j: None, None)
    training._complete_hyps(_hyps(ppo_epochs=2, gauss_loss="reference", is_discrete=True, action_size=2), lambda j: None, None)
