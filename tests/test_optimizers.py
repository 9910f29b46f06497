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
