#!/usr/bin/env python3
"""Measures the Snake worlds in device memory (csrc/snake.hip, a2c_amd.snake.DeviceSnakePool) on one MI355X:

  * a2c_snake_step: microseconds per launch at B = 32, 256, 2048 (default 15x15 world and the 84x84 one, grid_size=21);
  * env-steps/s of a full epoch (rollout + update, RMSprop) with DeviceSnakePool: FCModel on the default world and
    A3CModel on the 84x84 world.

Method: everything that allocates or tunes runs in a warm-up; a sample times `--iters` back-to-back launches (or
`--epochs` epochs) between two HIP events on the launch stream, so launch gaps are included the way a training run
sees them; `--repeats` samples, the median is reported with min and max beside it.  Actions of the kernel timing are
pre-drawn uniform ones (worlds die and reset often: the reset path is part of the average).  One JSON line on stdout.

    python tools/snake_bench.py [--iters 2000] [--epochs 30] [--repeats 5] [--n-envs 256]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-a2c_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

WORLDS = {"15x15x4": dict(grid_size=15, unit_size=4, n_foods=2), "21x21x4": dict(grid_size=21, unit_size=4, n_foods=2)}


def timed(fn, n, repeats):
    """median / min / max milliseconds of `n` calls of fn, over `repeats` samples"""
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _i in range(n):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def bench_step(world, B, iters, repeats):
    from a2c_amd.snake import DeviceSnakePool
    pool = DeviceSnakePool(B, "cuda", seed=1, **world)
    pool.reset()
    g = torch.Generator(device="cuda").manual_seed(3)
    acts = torch.randint(0, 4, (64, B), device="cuda", generator=g)
    k = [0]

    def one():
        pool.step(acts[k[0] & 63].data_ptr(), 1)
        k[0] += 1
    for _ in range(200):
        one()
    med, lo, hi = timed(one, iters, repeats)
    return dict(us=round(1e3 * med / iters, 3), us_min=round(1e3 * lo / iters, 3), us_max=round(1e3 * hi / iters, 3))


def bench_epoch(model, world, n_envs, T, epochs, repeats):
    import a2c_amd
    from a2c_amd.runner import Runner
    from a2c_amd.snake import DeviceSnakePool
    from a2c_amd.updater import Updater
    side = world["grid_size"] * world["unit_size"]
    ss = (4, side, side)
    hyps = dict(gamma=.99, lambda_=.98, n_tsteps=T, n_rollouts=n_envs, n_envs=n_envs, n_frame_stack=4, action_shift=0,
                render=False, env_type="Snake-device", use_bptt=False, use_nstep_rets=False, norm_advs=True,
                entr_coef=.005, pi_coef=1.0, val_coef=.5, max_norm=.5, lr=1e-4, optim_type="RMSprop", is_discrete=True,
                h_size=256, seed=0)
    torch.manual_seed(0)
    net = getattr(a2c_amd.models, model)(list(ss), 4, h_size=256)
    N = n_envs * T
    D = dict(states=torch.zeros(N, *ss, device="cuda"), deltas=torch.zeros(N, device="cuda"),
             rewards=torch.zeros(N, device="cuda"), dones=torch.zeros(N, device="cuda"),
             actions=torch.zeros(N, dtype=torch.int64, device="cuda"))
    r = Runner(D, hyps, None, None, None, env_pool=DeviceSnakePool(n_envs, "cuda", seed=1, **world))
    upd = Updater(net, hyps)
    slots = list(range(n_envs))

    def epoch():
        r.rollout(net, slots, hyps)
        upd.update_model(D)
    for _ in range(5):
        epoch()
    med, lo, hi = timed(epoch, epochs, repeats)
    f = lambda ms: round(N * epochs / (ms * 1e-3))
    return dict(model=model, n_envs=n_envs, n_tsteps=T, ms_per_epoch=round(med / epochs, 3), env_steps_per_s=f(med),
                env_steps_per_s_min=f(hi), env_steps_per_s_max=f(lo))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-envs", type=int, default=256)
    ap.add_argument("--n-tsteps", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "snake_bench needs the MI355X"
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, repeats=args.repeats, step={}, epoch={})
    for wn, w in WORLDS.items():
        for B in (32, 256, 2048):
            res["step"][f"{wn}_B{B}"] = bench_step(w, B, args.iters, args.repeats)
    res["epoch"]["FCModel_15x15x4"] = bench_epoch("FCModel", WORLDS["15x15x4"], args.n_envs, args.n_tsteps, args.epochs,
                                                   args.repeats)
    res["epoch"]["A3CModel_21x21x4"] = bench_epoch("A3CModel", WORLDS["21x21x4"], args.n_envs, args.n_tsteps, args.epochs,
                                                    args.repeats)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
