#!/usr/bin/env python3
"""Generate tests/golden/g11_snake_prep.npz FROM THE REFERENCE ITSELF: the reference's own ``snake_prep``
(a2c/preprocessing.py:25-32) on raw RGB frames that a2c_amd.snake.SnakeEnv produced (three worlds, a fixed action tape,
every frame kind: reset, move, food, the frame after a death), plus two hand-made pictures that mix the colour code with
other pixel values.  Runs only where the reference checkout is (build container).

preprocessing.py imports skimage.color.rgb2grey, which is not installed: it is stubbed exactly as make_golden.py's g9 does
(snake_prep never calls it).

    python tests/golden/make_golden_snake.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/a2c"
OUT = os.path.join(HERE, "g11_snake_prep.npz")
sys.path.insert(0, os.path.join(ROOT, "pytorch-a2c_amd"))

WORLDS = (dict(seed=11, env_id=0, grid_size=15, unit_size=4, n_foods=2),
          dict(seed=11, env_id=5, grid_size=21, unit_size=4, n_foods=3),
          dict(seed=7, env_id=2, grid_size=6, unit_size=2, n_foods=4))
N_STEPS = 6


def raw_frames():
    """name -> raw (H, W, 3) uint8 picture (what the tests feed to the project's snake_prep)"""
    from a2c_amd.snake import SnakeEnv, hash32
    out = {}
    for w, kw in enumerate(WORLDS):
        env = SnakeEnv(**kw)
        out[f"w{w}_f0"] = env.reset()
        for t in range(N_STEPS):
            obs, _, done, _ = env.step(hash32(99, w, t) & 3)
            if done:
                obs = env.reset()
            out[f"w{w}_f{t + 1}"] = obs
    rng = np.random.RandomState(5)
    out["mixed0"] = rng.randint(0, 256, size=(12, 10, 3)).astype(np.uint8)
    out["mixed1"] = rng.choice(np.array([0, 1, 255], dtype=np.uint8), size=(9, 16, 3))
    return out


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m


def build():
    def rgb2grey(a):
        raise AssertionError("stub: snake_prep does not call rgb2grey")
    _stub("skimage")
    _stub("skimage.color", rgb2grey=rgb2grey)
    spec = importlib.util.spec_from_file_location("a2c.preprocessing", os.path.join(REF, "preprocessing.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    out = {}
    for name, pic in raw_frames().items():
        y = np.array(m.snake_prep(pic.copy()))
        assert y.dtype == np.float32 and y.shape == (1,) + pic.shape[:2]
        out[name + "_raw"] = pic
        out[name + "_prep"] = y
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **build())
    print(OUT, os.path.getsize(OUT), "bytes")
