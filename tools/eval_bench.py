#!/usr/bin/env python3
"""Measures an evaluation of the device worlds on one MI355X: the host twins behind ``StatsRunner(hyps, envs=...)`` (what
``train()`` does by default) against ``DeviceStatsRunner`` (``hyps["eval_pool"] = "device"``).

  * one evaluation = 15 worlds, ``max_eval_steps`` = 2000, a fresh net (seed 0), the sampler's own uniforms; Pong and Breakout
    with their default worlds, each with FCModel and A3CModel;
  * ``eval_chunk`` 8, 16, 32, 64 on Pong with both models (device path);
  * milliseconds per ``train()`` epoch, 256 envs x 16 steps on Pong-device, with ``eval_pool`` host and device.

Method: ONE PROCESS PER SAMPLE (this script starts itself with --sample / --train-sample), the two paths alternating, so that
no sample inherits another's allocator, graphs or tuner state and drift of the shared host hits both paths alike.  A sample
makes one warm evaluation (allocations, tuners, the first capture), then times the next one with the host clock between two
device synchronisations -- an evaluation ends in a device read either way.  The device path's second call plays worlds
10022.. and the host twins go on from where their first episode ended: the two paths do not play the same episodes, so
beside the milliseconds every row carries the lock-step steps it played and the microseconds per step.  ``masked`` is
steps played minus the longest episode: what the last chunk played after the last env had finished.  A train() sample times
the epochs between ``on_epoch`` calls (update -> evaluation -> gate -> rollout -> update) and reports the median interval
after the first four.  Reported: median (min / max) over the samples.  One JSON line on stdout (and in --out).

    python tools/eval_bench.py [--samples 5] [--train-samples 3] [--train-epochs 14] [--skip eval,chunk,train] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-a2c_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

E, CAP = 15, 2000
WORLDS = {"pong": ("Pong-device", (4, 80, 80), 3), "breakout": ("Breakout-device", (4, 80, 72), 4)}


def hyps_for(world, chunk):
    return dict(gamma=.99, lambda_=.98, n_frame_stack=4, action_shift=0, render=False, env_type=WORLDS[world][0], is_discrete=True,
                h_size=256, seed=0, n_test_eps=E, max_eval_steps=CAP, eval_chunk=chunk)


def sample(world, model, path, chunk):
    """one process, one timed evaluation -> dict(ms, steps, longest, score)"""
    import torch
    import a2c_amd
    from a2c_amd import breakout, pong, preprocessing
    from a2c_amd.runner import DeviceStatsRunner, SequentialEnvironment, StatsRunner
    assert torch.cuda.is_available(), "eval_bench needs the MI355X"
    env_type, ss, n_act = WORLDS[world]
    hyps = hyps_for(world, chunk)
    torch.manual_seed(0)
    net = getattr(a2c_amd.models, model)(list(ss), n_act, h_size=256)
    mod = dict(pong=pong, breakout=breakout)[world]
    steps = [0]
    if path == "host":
        prep = getattr(preprocessing, world + "_prep")
        factory = mod.PongFactory if world == "pong" else mod.BreakoutFactory
        envs = [SequentialEnvironment(env_type, prep, seed=0, env_fn=factory(env_id=10007 + j, seed=0)) for j in range(E)]

        def uniforms(t, n):
            steps[0] = t + 1
            return torch.rand(n, device="cuda", dtype=torch.float32)
        sr = StatsRunner(hyps, envs=envs, uniform_fn=uniforms)
    else:
        pool = (mod.DevicePongPool if world == "pong" else mod.DeviceBreakoutPool)(E, "cuda", seed=0)
        sr = DeviceStatsRunner(hyps, pool)
    sr.rollout(net)                       # warm: allocations, tuners, the first capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    score = sr.rollout(net)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    if path == "host":
        return dict(ms=ms, steps=steps[0], longest=steps[0], score=score, device=torch.cuda.get_device_name(0))
    return dict(ms=ms, steps=sr.last["steps"], longest=int(sr.last["ep_len"].max()), chunks=sr.last["chunks"], score=score,
                device=torch.cuda.get_device_name(0))


def train_sample(model, eval_pool, epochs):
    """one process, one train() run -> dict(ms_per_epoch): the median interval between on_epoch calls after the first four"""
    import torch
    from a2c_amd.training import train
    assert torch.cuda.is_available(), "eval_bench needs the MI355X"
    stamps = []

    def on_epoch(epoch, upd, D):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
    with tempfile.TemporaryDirectory() as tmp:
        hyps = dict(exp_name="eval_bench", main_path=tmp, model=model, env_type="Pong-device", n_envs=256, n_rollouts=256,
                    n_tsteps=16, max_tsteps=1e12, seed=1, n_test_eps=E, max_eval_steps=CAP, eval_pool=eval_pool)
        train(None, hyps, verbose=False, max_epochs=epochs, on_epoch=on_epoch)
    d = [1e3 * (b - a) for a, b in zip(stamps[4:], stamps[5:])]
    return dict(ms_per_epoch=statistics.median(d), ms_min=min(d), ms_max=max(d), epochs_timed=len(d))


def child(args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(f"eval_bench {' '.join(args)} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def mmm(xs, nd=3):
    return dict(median=round(statistics.median(xs), nd), min=round(min(xs), nd), max=round(max(xs), nd))


def summarise(rows):
    """samples of one (configuration, path) -> median (min / max) ms, the steps played, us per lock-step step"""
    out = dict(ms=mmm([r["ms"] for r in rows]), steps=[r["steps"] for r in rows],
               us_per_step=mmm([1e3 * r["ms"] / max(r["steps"], 1) for r in rows], 2), score=[round(r["score"], 4) for r in rows])
    if "chunks" in rows[0]:
        out["masked_steps"] = [r["steps"] - r["longest"] for r in rows]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--train-samples", type=int, default=3)
    ap.add_argument("--train-epochs", type=int, default=14)
    ap.add_argument("--skip", default="", help="comma list of eval, chunk, train")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sample", nargs=4, metavar=("WORLD", "MODEL", "PATH", "CHUNK"), help="(internal) one evaluation sample")
    ap.add_argument("--train-sample", nargs=3, metavar=("MODEL", "EVAL_POOL", "EPOCHS"), help="(internal) one train() sample")
    args = ap.parse_args()
    if args.sample:
        w, m, p, c = args.sample
        print(json.dumps(sample(w, m, p, int(c))))
        return
    if args.train_sample:
        m, p, n = args.train_sample
        print(json.dumps(train_sample(m, p, int(n))))
        return
    skip = set(filter(None, args.skip.split(",")))
    res = dict(device=None, n_test_eps=E, max_eval_steps=CAP, samples=args.samples, evaluation={}, eval_chunk={}, train_epoch={})
    if "eval" not in skip:
        for world in WORLDS:
            for model in ("FCModel", "A3CModel"):
                rows = dict(host=[], device=[])
                for _ in range(args.samples):
                    for path in ("host", "device"):
                        rows[path].append(child(["--sample", world, model, path, "32"]))
                        res["device"] = rows[path][-1]["device"]
                res["evaluation"][f"{world}/{model}"] = {p: summarise(r) for p, r in rows.items()}
                print(f"{world}/{model}: {json.dumps(res['evaluation'][f'{world}/{model}'])}", file=sys.stderr, flush=True)
    if "chunk" not in skip:
        for model in ("FCModel", "A3CModel"):
            rows = {c: [] for c in (8, 16, 32, 64)}
            for _ in range(args.samples):
                for c in rows:
                    rows[c].append(child(["--sample", "pong", model, "device", str(c)]))
            res["eval_chunk"][f"pong/{model}"] = {str(c): summarise(r) for c, r in rows.items()}
            print(f"eval_chunk pong/{model}: {json.dumps(res['eval_chunk'][f'pong/{model}'])}", file=sys.stderr, flush=True)
    if "train" not in skip:
        for model in ("FCModel", "A3CModel"):
            rows = dict(host=[], device=[])
            for _ in range(args.train_samples):
                for pool in ("host", "device"):
                    rows[pool].append(child(["--train-sample", model, pool, str(args.train_epochs)]))
            res["train_epoch"][f"pong/{model}"] = {p: dict(ms_per_epoch=mmm([r["ms_per_epoch"] for r in r_]),
                                                              epochs_timed=r_[0]["epochs_timed"]) for p, r_ in rows.items()}
            print(f"train pong/{model}: {json.dumps(res['train_epoch'][f'pong/{model}'])}", file=sys.stderr, flush=True)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
