#!/usr/bin/env python3
"""Time the capturable (device-scalar) optimiser step against the host-scalar one, and a graphed Adam update against the
eager one.

Kernels, at the trainable arena of the headline A3CModel (Pong, 3 actions), for Adam, AdamW, Adamax, NAdam, RAdam, ASGD:
  host_step_us      a2c_clip_<name>: step-dependent scalars as launch arguments (the only path before capturable=True)
  dev_step_us       a2c_clip_step_dev: the same kernel body, scalars read from the device block
  advance_us        a2c_optim_advance alone (one wavefront): what the second launch of a capturable step costs
Each figure is the median of `--samples` samples; a sample brackets `--iters` back-to-back launches with HIP events, so it
holds the launch-to-launch time of a busy stream, as the update's own tail does.  The min and max of the samples are kept
beside the median: two figures closer than those spreads are not told apart by this run.

Update, A3CModel 256 slots x 128 steps, Adam: `eager_update_ms` (update_model, capturable=False: every launch issued by
the host) against `graphed_replay_ms` (capturable=True, capture_update + replay) and `eager_capturable_update_ms`.

    python tools/optim_capturable_bench.py --out profiles/optim_capturable_bench.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pytorch-a2c_amd")]

SIX = ("Adam", "AdamW", "Adamax", "NAdam", "RAdam", "ASGD")
HYPER = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, momentum_decay=4e-3, lambd=1e-4, alpha=0.75,
             t0=1e6)


def _timed(fn, samples, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / iters)
    return dict(median=round(statistics.median(us), 3), min=round(min(us), 3), max=round(max(us), 3))


def kernels(n, samples, iters, warmup):
    import torch
    from a2c_amd import ops
    from optim_bench import launcher
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.rand(n, device=dev, generator=gen) - 0.5
    g = (torch.rand(n, device=dev, generator=gen) - 0.5) * 1e-3
    s = [torch.zeros(n, device=dev) for _ in range(2)]
    sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
    norm = torch.zeros(1, device=dev)
    ops.gradnorm_sq(g, sumsq)
    rows = []
    for name in SIX:
        kind = ops.OPTIM_KINDS[name]
        blk = ops.optim_block_new(dev)
        ops.optim_block_set(blk, 0, 1.0, HYPER["lr"], 1.0)
        advance = lambda: ops.optim_advance(kind, blk, *HYPER.values())                                  # noqa: E731
        advance()
        step = lambda: ops.clip_step_dev(kind, p, g, s[0], None if name == "ASGD" else s[1], sumsq, 1e30, blk, norm)  # noqa: E731
        arrays = 1 if name == "ASGD" else 2
        row = dict(optimizer=name, n=n, bytes=n * (16 + 8 * arrays),
                   host_step_us=_timed(launcher(ops, name, p, g, s, sumsq, norm), samples, iters, warmup),
                   dev_step_us=_timed(step, samples, iters, warmup),
                   advance_us=_timed(advance, samples, iters, warmup))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def update(samples, iters, warmup, slots, T):
    import torch
    import a2c_amd
    from a2c_amd.updater import Updater
    dev = "cuda"
    N = slots * T
    gen = torch.Generator(device=dev).manual_seed(1)
    D = dict(states=(torch.rand(N, 4, 84, 84, device=dev, generator=gen) < 0.1).float(),
             rewards=torch.randint(-1, 2, (N,), device=dev, generator=gen).float(),
             deltas=torch.rand(N, device=dev, generator=gen) * 2 - 1,
             actions=torch.randint(0, 3, (N,), device=dev, generator=gen),
             dones=(torch.rand(N, device=dev, generator=gen) < 0.01).float())
    D["dones"][T - 1::T] = 1.0
    out = dict(model="A3CModel", slots=slots, n_tsteps=T, optimizer="Adam")

    def make(capturable):
        torch.manual_seed(0)
        net = a2c_amd.A3CModel([4, 84, 84], 3, h_size=256)
        hyps = dict(gamma=.99, lambda_=.98, n_tsteps=T, n_rollouts=slots, use_bptt=False, use_nstep_rets=False,
                    norm_advs=True, entr_coef=.005, pi_coef=1.0, val_coef=.5, max_norm=.5, lr=1e-4, optim_type="Adam",
                    is_discrete=True, h_size=256, optim_capturable=capturable)
        upd = Updater(net, hyps)
        upd.update_model(D)
        return upd

    def ms(t):
        return {k: round(v / 1e3, 4) for k, v in t.items()}

    upd = make(False)
    out["eager_update_ms"] = ms(_timed(lambda: upd.update_model(D), samples, iters, warmup))
    del upd
    upd = make(True)
    out["eager_capturable_update_ms"] = ms(_timed(lambda: upd.update_model(D), samples, iters, warmup))
    rep = upd.capture_update(D)
    out["graphed_replay_ms"] = ms(_timed(rep.replay, samples, iters, warmup))
    out["graph_fallbacks"] = rep.fallbacks
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--tsteps", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_capturable_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from optim_bench import headline_n_train
    doc = dict(tool="tools/optim_capturable_bench.py", samples=a.samples, iters=a.iters, warmup=a.warmup,
               timing="HIP events around `iters` back-to-back calls; median / min / max over `samples` samples",
               kernels=kernels(headline_n_train(), a.samples, a.iters, a.warmup),
               update=update(a.samples, max(a.iters // 5, 5), max(a.warmup // 2, 3), a.slots, a.tsteps))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
