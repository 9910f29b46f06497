"""The optimiser registry and the argument checks of the fused clip + step entry points (no GPU needed).  The
arithmetic is checked on the GPU in test_gpu_optimizers.py against torch.optim and the oracle."""
from ctypes import c_double, c_int64, c_void_p

import pytest
import torch

import a2c_amd
from a2c_amd import _lib, optim as fused_optim
from a2c_amd.updater import Updater
from cases import base_hyps

NEW = ("SGD", "Adagrad", "Adadelta", "Rprop", "AdamW", "Adamax", "NAdam", "RAdam", "ASGD")
ENTRY = {n: "a2c_clip_" + n.lower() for n in NEW}


def test_registry_holds_the_eleven_names():
    assert set(fused_optim.OPTIMIZERS) == {"RMSprop", "Adam", *NEW}
    for name, cls in fused_optim.OPTIMIZERS.items():
        assert cls.__name__ == name and issubclass(cls, torch.optim.Optimizer)


@pytest.mark.parametrize("name", ["LBFGS", "SparseAdam", "Adafactor", "Muon", "Nope"])
def test_unsupported_names_raise_before_device_work(name):
    net = a2c_amd.FCModel([4], 2, h_size=16)
    with pytest.raises(ValueError, match="not supported") as e:
        Updater(net, base_hyps(optim_type=name))
    for ok in fused_optim.OPTIMIZERS:
        assert ok in str(e.value)
    assert net._arena is None                     # nothing was put on a device


@pytest.mark.parametrize("name", NEW)
def test_supported_names_reach_the_optimiser(name):
    """the name is looked up in the registry: without a GPU the optimiser then asks for the device (before this, the
    nine names failed with an AttributeError); with one it is built"""
    net = a2c_amd.FCModel([4], 2, h_size=16)
    try:
        upd = Updater(net, base_hyps(optim_type=name))
    except RuntimeError as e:
        assert "HIP device" in str(e)
    else:
        assert type(upd.optim).__name__ == name


def _args(name, n=16, arrays=None, sumsq=64, step=1):
    """positional arguments of an a2c_clip_* call: the arrays before n, sumsq right after it, every other pointer
    (norm_out, stream) NULL, every double 0.5, every later int64 (the step) = step"""
    argtypes = _lib.SIGNATURES[name][1]
    i_n = argtypes.index(c_int64)
    out = list(arrays if arrays is not None else [64 * (k + 1) for k in range(i_n)])
    out.append(n)
    for k, t in enumerate(argtypes[i_n + 1:], i_n + 1):
        if t is c_void_p:
            out.append(sumsq if k == i_n + 1 else None)
        elif t is c_double:
            out.append(0.5)
        else:
            out.append(step)
    return out, i_n


@pytest.mark.parametrize("opt", NEW)
def test_entry_points_validate_like_clip_adam(opt):
    lib = _lib.load()
    name = ENTRY[opt]
    fn = getattr(lib, name)
    args, n_arrays = _args(name)
    assert n_arrays == 2 + len(fused_optim.OPTIMIZERS[opt]._state_names)
    # n == 0: a no-op (nothing is launched), with or without arrays
    assert fn(*_args(name, n=0)[0]) == 0
    assert fn(*_args(name, n=0, arrays=[None] * n_arrays)[0]) == 0
    assert fn(*_args(name, n=-1)[0]) == -1
    assert fn(*_args(name, sumsq=None)[0]) == -1
    for k in range(n_arrays):
        arrs = [64 * (j + 1) for j in range(n_arrays)]
        arrs[k] = None
        assert fn(*_args(name, arrays=arrs)[0]) == -1, (name, "NULL", k)
        arrs[k] = 64 * (k + 1) + 4                # not 16-B aligned
        assert fn(*_args(name, arrays=arrs)[0]) == -1, (name, "misaligned", k)
    if c_int64 in _lib.SIGNATURES[name][1][n_arrays + 1:]:        # takes a 1-based step count
        assert fn(*_args(name, step=0)[0]) == -1


def test_header_declares_the_new_entry_points():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "a2c_mi355x.h")).read()
    for name in ENTRY.values():
        assert f"int {name}(" in src


def test_nadam_and_asgd_scalar_chains_equal_torch_for_3000_steps():
    """the fp32 scalars the NAdam / ASGD classes carry from step to step on the host (optim.nadam_mu_product,
    optim.asgd_eta_mu: what their _launch calls) against the 0-d state tensors of torch.optim on a 4-element CPU
    tensor: exact equality at every step (mu_product reaches 0.0 in fp32 near step 1000, in torch too)"""
    def stepped(opt_cls, **group):
        p = torch.zeros(4, requires_grad=True)
        opt = opt_cls([p])
        opt.param_groups[0].update(group)
        for step in range(1, 3001):
            p.grad = torch.full((4,), 1e-3)
            opt.step()
            yield step, opt.param_groups[0], opt.state[p]

    mu_product = 1.0
    for step, grp, st in stepped(torch.optim.NAdam):
        mu_product = fused_optim.nadam_mu_product(mu_product, step, grp["betas"][0], grp["momentum_decay"])
        assert mu_product == float(st["mu_product"]), step
    assert mu_product == 0.0
    for t0 in (1e6, 2.0, 100.0):
        mus = set()
        for step, grp, st in stepped(torch.optim.ASGD, t0=t0):
            eta, mu = fused_optim.asgd_eta_mu(step, grp["lr"], grp["lambd"], grp["alpha"], grp["t0"])
            assert (eta, mu) == (float(st["eta"]), float(st["mu"])), (t0, step)
            mus.add(mu)
        assert len(mus) == (1 if t0 == 1e6 else 3000 - int(t0))
