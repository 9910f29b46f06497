#!/usr/bin/env python3
"""Measures the Breakout worlds in device memory (csrc/breakout.hip, a2c_amd.breakout.DeviceBreakoutPool) on one MI355X:

  * a2c_breakout_step: microseconds per launch at B = 32, 256, 2048;
  * env-steps/s of a full epoch (rollout + update, RMSprop) with DeviceBreakoutPool for FCModel and A3CModel (80 x 72 frames:
    the generic conv route), and how many launches Python issues per epoch through the ctypes binding;
  * a2c_breakout_step + a2c_rollout_post against a2c_breakout_step_post (the same work in one launch): GPU microseconds per env
    step at B = 32, 256, 2048, timed INSIDE a replayed hipGraph of 200 steps, so that the figure is kernel time and not the
    rate at which the binding issues launches;
  * --graphs on|off: the epochs with the Runner's one-graph device slot (the default of hyps["rollout_graphs"]) or with
    its eager loop;
  * with --learn N: a learning sanity run -- N epochs on 64 device worlds with the reference's coefficients, then the
    sampled policy's reward per step on fresh device worlds against the uniform-random policy's on the host twins of the
    same worlds, with the standard error of the difference (envs are the independent units).

Method: everything that allocates or tunes runs in a warm-up; a sample times `--iters` back-to-back launches (or
`--epochs` epochs) between two HIP events on the launch stream, so launch gaps are included the way a training run
sees them; `--repeats` samples, the median is reported with min and max beside it.  Actions of the kernel timing are
pre-drawn uniform ones.  One JSON line on stdout.

    python tools/breakout_bench.py [--iters 2000] [--epochs 30] [--repeats 5] [--n-envs 256] [--graphs on|off] [--learn 0]
                               [--frame-skip 1] [--sticky 0/1] [--frame-skip-max K] [--episodic-life] [--clip-rewards]

--frame-skip K / --sticky NUM/DEN measure worlds that play K game frames per env step with sticky actions (DESIGN.md section
6g; the learning run keeps the plain world): the epochs then report game frames/s = K x env-steps/s beside env-steps/s.
--frame-skip-max M draws the game frames of every env step from K .. M (section 6i; game frames/s then takes the mean
(K + M) / 2, what the draw gives on average when no step is cut); --episodic-life / --clip-rewards are the Breakout worlds'
training flags of that section.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_ACT, FRAME = 4, (80, 72)


REPEAT = {}      # --frame-skip / --sticky / --frame-skip-max / --episodic-life / --clip-rewards: the keywords of the measured pools


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


def bench_step(B, iters, repeats):
    from a2c_amd.breakout import DeviceBreakoutPool
    pool = DeviceBreakoutPool(B, "cuda", seed=1, **REPEAT)
    pool.reset_all()
    g = torch.Generator(device="cuda").manual_seed(3)
    acts = torch.randint(0, N_ACT, (64, B), device="cuda", generator=g)
    k = [0]

    def one():
        pool.step(acts[k[0] & 63].data_ptr(), 1)
        k[0] += 1
    for _ in range(200):
        one()
    med, lo, hi = timed(one, iters, repeats)
    return dict(us=round(1e3 * med / iters, 3), us_min=round(1e3 * lo / iters, 3), us_max=round(1e3 * hi / iters, 3))


def bench_step_post(B, repeats, steps=200, C=4):
    """GPU microseconds per env step of [a2c_breakout_step + a2c_rollout_post] and of a2c_breakout_step_post: `steps` steps captured
    into one hipGraph each (states ping-pong between two (B, C*HW) buffers), the replay timed between two HIP events"""
    from a2c_amd import ops
    from a2c_amd.breakout import DeviceBreakoutPool
    g = torch.Generator(device="cuda").manual_seed(3)
    acts = torch.randint(0, N_ACT, (64, B), device="cuda", generator=g)
    out = {}
    for name in ("step_then_post", "step_post"):
        pool = DeviceBreakoutPool(B, "cuda", seed=1, **REPEAT)
        pool.reset_all()
        HW = pool.HW
        S = C * HW
        x = [torch.zeros((B, S), device="cuda") for _ in range(2)]
        rewards, dones, deltas = (torch.zeros(2 * B, device="cuda") for _ in range(3))
        val, val_prev = torch.rand(B, device="cuda"), torch.zeros(B, device="cuda")

        def play():
            for i in range(steps):
                a, prev, nxt = acts[i & 63].data_ptr(), x[i & 1].data_ptr(), x[1 - (i & 1)].data_ptr()
                if name == "step_post":
                    post = ops.world_post(val.data_ptr(), 1, val_prev, rewards, dones, deltas, 2, 1, 0, .99, False, prev, S, nxt, S, C)
                    pool.device_step_post(1, 0, B, (a, 1), post)
                else:
                    fr, rew, done, reset = pool.device_step(1, 0, B, actions=(a, 1))
                    ops.rollout_post(rew, done, val.data_ptr(), 1, val_prev, rewards, dones, deltas, 2, 1, 0, .99, False, fr, reset,
                                     prev, S, nxt, S, B, C, HW)
        play()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with ops.graph_capture(graph):
            play()
        for _ in range(3):
            graph.replay()
        med, lo, hi = timed(graph.replay, 1, repeats)
        out[name] = dict(us=round(1e3 * med / steps, 3), us_min=round(1e3 * lo / steps, 3), us_max=round(1e3 * hi / steps, 3))
    return out


def hyps_for(n_envs, T, n_frame_stack=4):
    return dict(gamma=.99, lambda_=.98, n_tsteps=T, n_rollouts=n_envs, n_envs=n_envs, n_frame_stack=n_frame_stack,
                action_shift=0, render=False, env_type="Breakout-device", use_bptt=False, use_nstep_rets=False, norm_advs=True,
                entr_coef=.005, pi_coef=1.0, val_coef=.5, max_norm=.5, lr=1e-4, optim_type="RMSprop", is_discrete=True,
                h_size=256, seed=0)


def datas(N, ss):
    return dict(states=torch.zeros(N, *ss, device="cuda"), deltas=torch.zeros(N, device="cuda"),
                rewards=torch.zeros(N, device="cuda"), dones=torch.zeros(N, device="cuda"),
                actions=torch.zeros(N, dtype=torch.int64, device="cuda"))


class CountedLib:
    """the ctypes library with every call of a launching a2c_* entry point counted"""

    def __init__(self, lib):
        self._lib, self.n = lib, 0

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("a2c_") or name.endswith(("_bytes", "_supported", "_splits", "_version", "_string")):
            return f                              # size and capability queries launch nothing

        def counted(*a):
            self.n += 1
            return f(*a)
        return counted


def bench_epoch(model, n_envs, T, epochs, repeats, graphs=True):
    import a2c_amd
    from a2c_amd import ops
    from a2c_amd.breakout import DeviceBreakoutPool
    from a2c_amd.runner import Runner
    from a2c_amd.updater import Updater
    ss = (4,) + FRAME
    hyps = dict(hyps_for(n_envs, T), rollout_graphs=graphs)
    torch.manual_seed(0)
    net = getattr(a2c_amd.models, model)(list(ss), N_ACT, h_size=256)
    N = n_envs * T
    D = datas(N, ss)
    r = Runner(D, hyps, None, None, None, env_pool=DeviceBreakoutPool(n_envs, "cuda", seed=1, **REPEAT))
    upd = Updater(net, hyps)
    slots = list(range(n_envs))

    def epoch():
        r.rollout(net, slots, hyps)
        upd.update_model(D)
    for _ in range(5):
        epoch()
    med, lo, hi = timed(epoch, epochs, repeats)
    # launches per epoch: count the binding's calls over one more epoch
    real, counted = ops.lib, None
    try:
        counted = CountedLib(real())
        ops.lib = lambda: counted
        epoch()
        torch.cuda.synchronize()
    finally:
        ops.lib = real
    f = lambda ms: round(N * epochs / (ms * 1e-3))
    k = REPEAT.get("frame_skip", 1)
    k = (k + REPEAT.get("frame_skip_max", k)) / 2
    return dict(model=model, n_envs=n_envs, n_tsteps=T, rollout_graphs=graphs, ms_per_epoch=round(med / epochs, 3), env_steps_per_s=f(med),
                game_frames_per_s=round(k * f(med)), game_frames_per_s_min=round(k * f(hi)), game_frames_per_s_max=round(k * f(lo)),
                env_steps_per_s_min=f(hi), env_steps_per_s_max=f(lo), launches_issued_per_epoch=counted.n)


def learn(model, epochs, B=64, T=12, eval_envs=64, eval_T=50, eval_rounds=5):
    """reward per step of the sampled policy after `epochs` epochs against the uniform-random policy, on fresh worlds"""
    import time
    import a2c_amd
    from a2c_amd.breakout import BreakoutEnv, DeviceBreakoutPool
    from a2c_amd.runner import Runner
    from a2c_amd.snake import hash32
    from a2c_amd.updater import Updater
    ss = (3,) + FRAME
    hyps = hyps_for(B, T, n_frame_stack=3)
    torch.manual_seed(0)
    net = getattr(a2c_amd.models, model)(list(ss), N_ACT, h_size=256)
    D = datas(B * T, ss)
    r = Runner(D, hyps, None, None, None, env_pool=DeviceBreakoutPool(B, "cuda", seed=100))
    upd = Updater(net, hyps)
    t0 = time.time()
    for _ in range(epochs):
        r.rollout(net, list(range(B)), hyps)
        r.finish()
        upd.update_model(D)
    torch.cuda.synchronize()
    train_s = time.time() - t0
    eval_seed = 4242
    ehyps = dict(hyps, n_tsteps=eval_T, n_rollouts=eval_envs, n_envs=eval_envs)
    De = datas(eval_envs * eval_T, ss)
    re_ = Runner(De, ehyps, None, None, None, env_pool=DeviceBreakoutPool(eval_envs, "cuda", seed=eval_seed))
    for _ in range(eval_rounds):
        re_.rollout(net, list(range(eval_envs)), ehyps)
        re_.finish()
    n = eval_T * eval_rounds
    # the rollout's reward rows carry the bootstrap value in their last step: take the points from the worlds' own
    # reward-since-the-last-done word.  No episode ends inside the evaluation: while |vy| = 1 a life lasts at least 62
    # steps (12 up from the serve, 50 down from the wall), so five lives outlast the n = 250 steps
    st = re_.env_pool.state.cpu().numpy()
    assert (st[:, 8] == n).all() and (st[:, 9] == n).all(), "an evaluation episode ended"
    trained = st[:, 10].astype(np.float64) / n
    rand = np.zeros(eval_envs)
    for j in range(eval_envs):
        e = BreakoutEnv(seed=eval_seed, env_id=j)
        e.new_episode()
        for t in range(n):
            rew, done = e.advance(hash32(eval_seed ^ 0x5EED, j, t) % N_ACT)
            rand[j] += rew
            assert not done
    rand /= n
    se = float(np.sqrt(trained.var(ddof=1) / eval_envs + rand.var(ddof=1) / eval_envs))
    return dict(model=model, epochs=epochs, n_envs=B, n_tsteps=T, train_seconds=round(train_s, 2), eval_steps=eval_envs * n,
                trained=round(float(trained.mean()), 5), random=round(float(rand.mean()), 5),
                diff=round(float(trained.mean() - rand.mean()), 5), se=round(se, 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-envs", type=int, default=256)
    ap.add_argument("--n-tsteps", type=int, default=16)
    ap.add_argument("--graphs", choices=("on", "off"), default="on", help="the Runner's one-graph device slot, or its eager loop")
    ap.add_argument("--learn", type=int, default=0, help="epochs of the learning sanity run (0: skip it)")
    ap.add_argument("--learn-model", default="FCModel")
    ap.add_argument("--frame-skip", type=int, default=1, help="game frames per env step (DESIGN.md section 6g)")
    ap.add_argument("--sticky", default="0/1", metavar="NUM/DEN", help="probability that a game frame keeps the previous action")
    ap.add_argument("--frame-skip-max", type=int, default=None, help="draw the game frames per env step from frame-skip .. this "
                    "(DESIGN.md section 6i)")
    ap.add_argument("--episodic-life", action="store_true", help="a lost life closes the env step (Breakout worlds)")
    ap.add_argument("--clip-rewards", action="store_true", help="the env step's reward is its sign (Breakout worlds)")
    args = ap.parse_args()
    num, den = (int(v) for v in args.sticky.split("/"))
    if (args.frame_skip, num) != (1, 0):
        REPEAT.update(frame_skip=args.frame_skip, sticky_num=num, sticky_den=den)
    if args.frame_skip_max is not None:
        REPEAT.update(frame_skip=args.frame_skip, frame_skip_max=args.frame_skip_max)
    if args.episodic_life or args.clip_rewards:
        REPEAT.update(episodic_life=args.episodic_life, clip_rewards=args.clip_rewards)
    assert torch.cuda.is_available(), "breakout_bench needs the MI355X"
    from a2c_amd.breakout import DeviceBreakoutPool as DevicePool
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, repeats=args.repeats, graphs=args.graphs, frame_skip=args.frame_skip,
               sticky=args.sticky, frame_skip_max=args.frame_skip_max, episodic_life=args.episodic_life, clip_rewards=args.clip_rewards,
               step={}, epoch={})
    for B in (32, 256, 2048):
        res["step"][f"B{B}"] = bench_step(B, args.iters, args.repeats)
    if hasattr(DevicePool, "device_step_post"):
        res["step_post_in_graph"] = {f"B{B}": bench_step_post(B, args.repeats) for B in (32, 256, 2048)}
    for model in ("FCModel", "A3CModel"):
        res["epoch"][model] = bench_epoch(model, args.n_envs, args.n_tsteps, args.epochs, args.repeats, args.graphs == "on")
    if args.learn:
        res["learn"] = learn(args.learn_model, args.learn)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
