#!/usr/bin/env python3
"""Generate tests/golden/g10_continuous.npz FROM THE REFERENCE ITSELF: continuous (Gaussian) action spaces on FCModel and
GRUFCModel -- model forwards, a rollout and update_model.

Runs only in the build container (needs the reference checkout, imported by make_golden.load_reference under its stubs).
The reference's continuous update hard-codes ``actions.cuda()``: ``torch.Tensor.cuda`` is stubbed to the identity so that
it runs on the CPU.  ``torch.randn_like`` (the reference's get_action noise) is replaced by closed-form values
(cont_cases.rollout_noise) that the tests feed to the HIP rollout through ``Runner(normal_fn=...)``.  The env is
cont_cases.ContEnv behind a stubbed ``gym.make``.  The fixture holds numbers only.

    python tests/golden/make_golden_continuous.py
"""
import os
import queue
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (imports the reference under its stubs)
import cont_cases as CC  # noqa: E402

R = MG.R
OUT = os.path.join(HERE, "g10_continuous.npz")


def _ref_net(kind, n, h, raw_bias):
    net = getattr(R["models"], kind)(list(CC.STATE_SHAPE), n, h_size=h, bnorm=False, is_discrete=False)
    sd = CC.state_dict(kind, n, h, raw_bias)
    assert set(net.state_dict()) == set(sd), set(net.state_dict()) ^ set(sd)
    net.load_state_dict(sd)
    return net


def forwards(out):
    for i, (kind, n, h, B) in enumerate(CC.MODEL_CASES):
        net = _ref_net(kind, n, h, CC.RAW_BIAS[n])
        x, hin = CC.model_input(i, kind, B, h)
        with torch.no_grad():
            if hin is not None:
                v, (mu, sg), hn = net(x, hin)
                out[f"fwd{i}_h"] = hn.numpy()
            else:
                v, (mu, sg) = net(x)
        out[f"fwd{i}_val"], out[f"fwd{i}_mu"], out[f"fwd{i}_sigma"] = v.numpy(), mu.numpy(), sg.numpy()
        out[f"fwd{i}_shapes"] = np.array([f"{k}:{tuple(t.shape)}" for k, t in net.state_dict().items()])


def rollouts(out):
    real_randn_like = torch.randn_like
    gym = sys.modules["gym"]
    for ci, (name, kind, n, h, T, B) in enumerate(CC.ROLLOUT_CASES):
        hyps = CC.cont_hyps(n_tsteps=T, n_rollouts=B)
        net = _ref_net(kind, n, h, CC.RAW_BIAS[n])
        N = T * B
        datas = dict(states=torch.zeros(N, *CC.STATE_SHAPE), deltas=torch.zeros(N), rewards=torch.zeros(N),
                     actions=torch.zeros(N, n), dones=torch.zeros(N))
        if net.is_recurrent:
            datas["h_states"] = torch.zeros(N, h)
        eps = CC.rollout_noise(ci, T, B, n)
        for j in range(B):              # env j plays slot j, like the HIP Runner's lock-step envs
            gym.make = lambda env_type, j=j: CC.ContEnv(n, env_id=j, done_period=4 + j)
            rew_q = queue.Queue(1)
            rew_q.put(-1)
            runner = R["runner"].Runner(datas, hyps, None, None, rew_q)
            runner.net = net
            runner.env = R["runner"].SequentialEnvironment(**hyps)
            runner.state_bookmark = R["utils"].next_state(runner.env, runner.obs_deque, obs=None, reset=True)
            runner.h_bookmark = torch.zeros(1, h) if net.is_recurrent else None
            runner.ep_rew = 0
            for p in net.parameters():
                p.requires_grad = False
            it = iter(eps[:, j])
            torch.randn_like = lambda s, it=it: torch.from_numpy(next(it).copy()).reshape(s.shape)
            try:
                runner.rollout(net, j, hyps)
            finally:
                torch.randn_like = real_randn_like
        out[f"{name}_noise"] = eps
        for k in ("states", "actions", "rewards", "dones", "deltas") + (("h_states",) if net.is_recurrent else ()):
            out[f"{name}_{k}"] = datas[k].numpy()


def updates(out):
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for ci, (name, kind, n, h, R_, T, opt, norm_advs) in enumerate(CC.UPDATE_CASES):
            net = _ref_net(kind, n, h, CC.UPDATE_RAW_BIAS[n])
            hyps = CC.cont_hyps(n_tsteps=T, n_rollouts=R_, optim_type=opt, norm_advs=norm_advs, h_size=h)
            upd = R["updater"].Updater(net, hyps)
            D = CC.synth_shared(n, h, R_, T, seed=1200 + 10 * ci, recurrent=net.is_recurrent)
            info = upd.update_model(D)
            for k, v in info.items():
                out[f"{name}_{k}"] = np.array(float(v))
            out[f"{name}_params"] = np.concatenate([p.detach().reshape(-1).numpy() for p in net.parameters()])
    finally:
        torch.Tensor.cuda = real_cuda


def build():
    torch.manual_seed(0)
    out = {}
    forwards(out)
    rollouts(out)
    updates(out)
    return out


if __name__ == "__main__":
    arrs = build()
    np.savez_compressed(OUT, **arrs)
    print(f"{os.path.basename(OUT)}: {os.path.getsize(OUT) / 1024:.1f} KiB, {len(arrs)} arrays")
