"""Continuous-action (Gaussian policy) cases shared by make_golden_continuous.py (which runs the REFERENCE on them, build
container only) and by tests/test_continuous.py / tests/test_gpu_continuous.py (which run the HIP path on the same
inputs).  Everything here is closed form; nothing comes from the reference."""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cases import O, base_hyps, hashf  # noqa: E402

D_OBS = 5            # observation length of ContEnv
C_STACK = 2          # n_frame_stack of the cases
STATE_SHAPE = (C_STACK, 1, D_OBS)


class BoxSpace:
    """what SequentialEnvironment reads of a gym ``Box``: ``shape`` and no ``n``"""

    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.inf * np.ones(n, np.float32), np.inf * np.ones(n, np.float32)


class ContEnv:
    """Closed-form continuous-control env: obs (1, D_OBS); reward -sum((a - target_t)^2) over the n action components;
    done every ``done_period`` steps.  ``prepped`` adds the leading plane axis a preprocessor would (null_prep)."""

    def __init__(self, n, env_id=0, done_period=7, prepped=False):
        self.n, self.env_id, self.done_period, self.prepped = n, env_id, done_period, prepped
        self.action_space = BoxSpace(n)
        self.t = 0
        self.actions = []

    def seed(self, s):
        pass

    def _obs(self):
        k = np.arange(D_OBS, dtype=np.float64)
        o = np.sin(0.37 * self.t + 0.61 * k + 1.3 * self.env_id).astype(np.float32)[None]
        return o[None] if self.prepped else o

    def target(self, t):
        return np.cos(0.23 * t + 0.5 * np.arange(self.n) + 0.7 * self.env_id)

    def reset(self):
        self.t = 0
        return self._obs()

    def step(self, a):
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        assert a.shape == (self.n,), a.shape
        self.actions.append(a.copy())
        rew = float(np.round(-np.sum((a - self.target(self.t)) ** 2), 4))
        self.t += 1
        done = self.t % self.done_period == 0
        return self._obs(), rew, done, {}


def state_dict(kind, n, h, raw_bias=None):
    """reference-keyed state_dict of a continuous FCModel / GRUFCModel (action_out 2n wide), by formula; raw_bias
    overrides the sigma half of action_out.bias (drives the softplus threshold and the clamp regimes)"""
    sd = O.formula_state_dict(kind, STATE_SHAPE, 2 * n, h)
    if raw_bias is not None:
        sd["action_out.bias"][n:] = torch.tensor(raw_bias, dtype=torch.float32)
    return sd


# raw columns per regime: > 20 (softplus identity), tiny sigma (both clamps), around the sigma^2 clamp, ordinary
RAW_BIAS = {1: [0.4], 2: [24.0, -9.0], 6: [-9.0, 21.5, -3.4, 0.2, -1.0, 3.0]}
# the update cases keep sigma off the clamps: a clamped column weights its rows by 1/(2c) = 500, and K = sum adv/(2c) over
# normalised advantages (which sum to zero) is then rounding noise -- in the reference as much as here -- that RMSprop /
# Adam's first step turns into lr-sized parameter differences.  The clamp regimes are checked at the loss level against a
# float64 statement instead (tests/test_gpu_continuous.py).  Likewise n == 1 with norm_advs weights every row by the mean
# of the normalised advantages, i.e. by rounding noise: the n == 1 update cases run without norm_advs.
UPDATE_RAW_BIAS = {1: [0.4], 2: [21.0, -0.8], 6: [0.3, 21.5, -1.2, 0.2, -1.0, 1.5]}

MODEL_CASES = [  # kind, n, h, batch
    ("FCModel", 1, 16, 5),
    ("FCModel", 2, 32, 7),
    ("FCModel", 6, 16, 3),
    ("GRUFCModel", 2, 16, 4),
    ("GRUFCModel", 6, 32, 3),
]

ROLLOUT_CASES = [  # name, kind, n, h, T, B (envs = slots)
    ("fc_n2", "FCModel", 2, 16, 6, 3),
    ("grufc_n1", "GRUFCModel", 1, 16, 5, 2),
]

UPDATE_CASES = [  # name, kind, n, h, R, T, optim, norm_advs
    ("fc_rms_n2", "FCModel", 2, 16, 3, 5, "RMSprop", True),
    ("fc_adam_n2", "FCModel", 2, 16, 3, 5, "Adam", True),
    ("fc_rms_n1", "FCModel", 1, 16, 4, 4, "RMSprop", False),
    ("fc_adam_n6_nonorm", "FCModel", 6, 16, 2, 6, "Adam", False),
    ("grufc_rms_n2", "GRUFCModel", 2, 16, 3, 4, "RMSprop", True),
    ("grufc_adam_n1_nonorm", "GRUFCModel", 1, 16, 2, 5, "Adam", False),
]

# GRUFCModel with use_bptt: the reference's bptt() does not accept the (mu, sigma) tuple, so these are checked against
# the public forward stepped over time (tests/test_gpu_continuous.py), not against recorded reference numbers
BPTT_CASES = [  # name, n, h, R, T, optim, norm_advs
    ("grufc_bptt_rms_n2", 2, 16, 3, 4, "RMSprop", True),
    ("grufc_bptt_rms_n1_nonorm", 1, 16, 2, 5, "RMSprop", False),
]


def cont_hyps(**kw):
    h = base_hyps(n_frame_stack=C_STACK, env_type="ContEnv", is_discrete=False, norm_advs=True)
    h.update(kw)
    return h


def model_input(i, kind, B, h):
    x = torch.from_numpy(hashf(B * C_STACK * D_OBS, 1000 + i, -1, 1).reshape(B, *STATE_SHAPE))
    hin = torch.from_numpy(hashf(B * h, 1050 + i, -1, 1).reshape(B, h)) if kind == "GRUFCModel" else None
    return x, hin


def rollout_noise(case_idx, T, B, n):
    """the closed-form stand-in for torch.randn_like of the reference's get_action: (T, B, n)"""
    return hashf(T * B * n, 1100 + case_idx, -2, 2).reshape(T, B, n)


def synth_shared(n, h, R_, T, seed, recurrent):
    """closed-form continuous shared_data: float (N, n) actions"""
    N = R_ * T
    D = dict(states=torch.from_numpy(hashf(N * C_STACK * D_OBS, seed, -1, 1).reshape(N, *STATE_SHAPE)),
             rewards=torch.from_numpy(hashf(N, seed + 1, -2, 0.5)),
             deltas=torch.from_numpy(hashf(N, seed + 2, -1, 1)),
             actions=torch.from_numpy(hashf(N * n, seed + 3, -1.5, 1.5).reshape(N, n)))
    d = (hashf(N, seed + 4) < 0.2).astype(np.float32)
    d[T - 1::T] = 1.0
    D["dones"] = torch.from_numpy(d)
    if recurrent:
        D["h_states"] = torch.from_numpy(hashf(N * h, seed + 5, -1, 1).reshape(N, h))
    return D


def gym_env_fn(n, env_id, done_period):
    """a gym-shaped factory: SequentialEnvironment(env_fn=...) takes raw (1, D_OBS) observations"""
    return types.SimpleNamespace(make=lambda: ContEnv(n, env_id=env_id, done_period=done_period))
