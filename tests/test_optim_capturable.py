"""CPU: the capturable Adam family's entry points and classes, as far as they go without a device."""
import inspect

import numpy as np
import pytest

from a2c_amd import _lib, ops, optim as fused_optim

SIX = ("Adam", "AdamW", "Adamax", "NAdam", "RAdam", "ASGD")


def test_block_layout_is_the_headers():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "a2c_mi355x.h")).read()
    assert int(re.search(r"#define A2C_OPTIM_BLOCK_BYTES (\d+)", src).group(1)) == ops.OPTIM_BLOCK_BYTES == 96
    body = re.search(r"typedef struct a2c_optim_block \{(.*?)\} a2c_optim_block;", src, flags=re.S).group(1)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert fields == list(ops.OPTIM_BLOCK_DTYPE.names)
    # the documented offsets
    for off, name in re.findall(r"^ \*\s+(\d+)\s+([a-z_0-9]+) ", src, flags=re.M):
        if name in ops.OPTIM_BLOCK_DTYPE.names:
            assert ops.OPTIM_BLOCK_DTYPE.fields[name][1] == int(off), name
    kinds = dict(re.findall(r"A2C_OPTIM_([A-Z]+) = (\d)", src))
    assert {k.upper(): v for k, v in ops.OPTIM_KINDS.items()} == {k: int(v) for k, v in kinds.items()}
    assert ops.OPTIM_BLOCK_DTYPE.itemsize % 16 == 0 and np.dtype("<i8").itemsize == 8


def test_entry_points_refuse_bad_blocks_and_arrays_before_launching():
    lib = _lib.load()
    adv = lambda kind, b: lib.a2c_optim_advance(kind, b, 1e-3, .9, .999, 1e-8, 0., 0., 0., 0., 0., None)   # noqa: E731
    assert adv(0, None) == -1 and adv(0, 4096 + 8) == -1 and adv(6, 4096) == -1 and adv(-1, 4096) == -1
    step = lambda kind, p, g, a, b, n, ss, blk: lib.a2c_clip_step_dev(kind, p, g, a, b, n, ss, 0.5, blk, None, None)  # noqa: E731
    ok = (64, 128, 192, 256)
    for kind in range(6):
        assert step(kind, *ok, 0, 512, 4096) == 0                        # n == 0: a no-op
        assert step(kind, None, None, None, None, 0, 512, 4096) == 0
        assert step(kind, *ok, -1, 512, 4096) == -1 and step(kind, *ok, 4, None, 4096) == -1
        assert step(kind, *ok, 4, 512, None) == -1 and step(kind, *ok, 4, 512, 4096 + 4) == -1
        for k in range(3 if kind == 5 else 4):                           # ASGD has one state array
            bad = list(ok)
            bad[k] = None
            assert step(kind, *bad, 4, 512, 4096) == -1, (kind, k)
            bad[k] = ok[k] + 4
            assert step(kind, *bad, 4, 512, 4096) == -1, (kind, k)
    assert step(6, *ok, 0, 512, 4096) == -1 and step(-1, *ok, 0, 512, 4096) == -1


def test_the_six_classes_take_capturable_and_the_others_do_not():
    for name, cls in fused_optim.OPTIMIZERS.items():
        has = "capturable" in inspect.signature(cls.__init__).parameters
        assert has == (name in SIX) == (cls._kind is not None), name
        if has:
            assert inspect.signature(cls.__init__).parameters["capturable"].default is False
            assert cls._kind == ops.OPTIM_KINDS[name] and cls.capture_safe is False
