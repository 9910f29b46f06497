"""hyps["gauss_loss"]: the host-side surface of the per-sample Gaussian log-likelihood loss -- the
key's validation in Updater and train(), and the a2c_gauss_nll_fwd_bwd binding.  No GPU needed; the numbers are checked on
the GPU in test_gpu_gauss_exact.py against a float64 autograd statement."""
import os
import re

import pytest
import torch

import a2c_amd
from a2c_amd import _lib
from a2c_amd.updater import Updater, gauss_loss_mode
import cont_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cont_net():
    return a2c_amd.FCModel(list(CC.STATE_SHAPE), 2, h_size=16, is_discrete=False)


def _construct(net, hyps):
    """Updater(net, hyps) as far as it gets without a device: past every hyps check, the optimiser needs the GPU"""
    if torch.cuda.is_available():
        return Updater(net, hyps)
    with pytest.raises(RuntimeError, match="HIP device"):
        Updater(net, hyps)
    return None


def test_key_values():
    assert gauss_loss_mode({}) == "reference"
    assert gauss_loss_mode({"gauss_loss": "reference"}, is_discrete=True) == "reference"
    assert gauss_loss_mode({"gauss_loss": "exact"}, is_discrete=False) == "exact"
    assert gauss_loss_mode({"gauss_loss": "exact"}) == "exact"           # action space not known yet
    for bad in ("Exact", "textbook", "", None, 1, True):
        with pytest.raises(ValueError, match="gauss_loss"):
            gauss_loss_mode({"gauss_loss": bad})
    with pytest.raises(ValueError, match="gauss_loss"):
        gauss_loss_mode({"gauss_loss": "exact"}, is_discrete=True)


def test_updater_accepts_reference_exact_and_a_missing_key():
    hyps = CC.cont_hyps()
    assert "gauss_loss" not in hyps
    for h, want in ((hyps, "reference"), (dict(hyps, gauss_loss="reference"), "reference"),
                    (dict(hyps, gauss_loss="exact"), "exact")):
        upd = _construct(_cont_net(), h)
        if upd is not None:
            assert upd.gauss_loss == want
            assert ("gsums" in upd._buffers(8)) == (want == "reference")      # "exact" does not allocate the six sums


def test_updater_refuses_a_bad_value_and_exact_on_a_discrete_net():
    with pytest.raises(ValueError, match="gauss_loss"):
        Updater(_cont_net(), CC.cont_hyps(gauss_loss="textbook"))
    disc = a2c_amd.FCModel(list(CC.STATE_SHAPE), 3, h_size=16)
    with pytest.raises(ValueError, match="gauss_loss"):
        Updater(disc, CC.cont_hyps(is_discrete=True, gauss_loss="exact"))
    with pytest.raises(ValueError, match="gauss_loss"):       # a bad value is refused on a discrete net too
        Updater(disc, CC.cont_hyps(is_discrete=True, gauss_loss="none"))
    _construct(disc, CC.cont_hyps(is_discrete=True, gauss_loss="reference"))


def _train_hyps(tmp_path, **kw):
    return dict(dict(exp_name="g", main_path=str(tmp_path), model="FCModel", env_type="ContEnv", n_envs=2, n_rollouts=2,
                     n_tsteps=3, max_tsteps=1e9, action_size=2, is_discrete=False, env_pool="serial", seed=1), **kw)


def test_train_refuses_before_anything_is_written(tmp_path):
    from a2c_amd.training import DEFAULTS, train
    assert DEFAULTS["gauss_loss"] == "reference"
    env_fn = lambda j: CC.ContEnv(2, env_id=j, prepped=True)
    with pytest.raises(ValueError, match="gauss_loss"):
        train(None, _train_hyps(tmp_path, gauss_loss="per-sample"), verbose=False, env_fn=env_fn, max_epochs=1)
    with pytest.raises(ValueError, match="gauss_loss"):       # an env_fn whose hyps say discrete
        train(None, _train_hyps(tmp_path, gauss_loss="exact", is_discrete=True), verbose=False, env_fn=env_fn, max_epochs=1)
    with pytest.raises(ValueError, match="gauss_loss"):       # a discrete device world
        train(None, _train_hyps(tmp_path, gauss_loss="exact", env_type="CartPole-device", is_discrete=True), verbose=False,
              max_epochs=1)
    assert os.listdir(str(tmp_path)) == []


def test_entry_point_is_bound_with_the_headers_parameter_count():
    src = open(os.path.join(ROOT, "include", "a2c_mi355x.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+a2c_gauss_nll_fwd_bwd\s*\(([^;{}]*?)\)\s*;", src, flags=re.S)
    assert m, "include/a2c_mi355x.h does not declare a2c_gauss_nll_fwd_bwd"
    params = [p.strip() for p in m.group(1).split(",") if p.strip()]
    assert params[-1].startswith("a2c_stream_t") and len(params) == 22
    res, args = _lib.SIGNATURES["a2c_gauss_nll_fwd_bwd"]
    assert res is _lib.c_int and len(args) == len(params)
    for ty, p in zip(args, params):       # pointers, 64-bit strides and counts, int n, the three float coefficients
        want = (_lib.P if "*" in p or p.startswith("a2c_stream_t") else _lib.c_int64 if p.startswith("int64_t") else
                _lib.c_float if p.startswith("float") else _lib.c_int)
        assert ty is want, p
    from a2c_amd import ops
    assert callable(ops.gauss_nll_fwd_bwd)


def test_entry_point_checks_its_arguments_without_a_device():
    lib = _lib.load()
    call = lambda n, ldh=200, ldd=200, lda=64, nl=4: lib.a2c_gauss_nll_fwd_bwd(
        None, ldh, None, 1, None, lda, None, None, None, nl, 4, n, 1.0, .5, .01, None, ldd, None, 1, None, None, None)
    assert call(0) == -1 and call(65) == -1 and call(3) == -1         # bad n; NULL sums / scratch
    buf = (_lib.c_double * 8)()
    import ctypes
    p = ctypes.cast(buf, ctypes.c_void_p)
    full = lambda n, ldh, ldd, lda, nl=4, ng=4: lib.a2c_gauss_nll_fwd_bwd(
        p, ldh, p, 1, p, lda, p, p, None, nl, ng, n, 1.0, .5, .01, p, ldd, p, 1, p, p, None)
    # (host addresses: every call below is refused before anything is launched)
    assert full(3, 5, 7, 3) == -1 and full(3, 7, 5, 3) == -1 and full(3, 7, 7, 2) == -1     # ld_heads, ldd < 2n; ld_act < n
    assert full(0, 7, 7, 3) == -1 and full(65, 200, 200, 65) == -1
    assert full(3, 7, 7, 3, nl=5, ng=4) == -1 and full(3, 7, 7, 3, nl=-1) == -1
    assert lib.a2c_gauss_nll_fwd_bwd(p, 7, p, 1, p, 3, p, p, p, 1, 1, 3, 1.0, .5, .01, p, 7, p, 1, p, p, None) == -1  # adv_sums, N < 2
    assert lib.a2c_gauss_nll_fwd_bwd(p, 7, p, 1, p, 3, p, p, None, 4, 4, 3, 1.0, .5, .01, None, 7, p, 1, p, p, None) == -1  # dheads
