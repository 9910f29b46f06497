#!/usr/bin/env python3
"""Measures the Pendulum worlds (csrc/pendulum.hip, a2c_amd.pendulum) on one MI355X:

  * ms per epoch and env-steps/s of a full epoch (rollout + update, RMSprop, 256 envs x 16 steps) for FCModel and
    GRUFCModel with Gaussian heads (one action), on four paths: ``DevicePendulumPool`` with the Runner's one-graph slot
    ("device_graph") and with its eager loop ("device_eager"), and ``PendulumEnv`` host twins stepped in this process
    ("host_serial") and by worker processes behind the float-action process pool ("host_process", ``process_f32``) -- the
    paths the device world is an alternative to;
  * a2c_pendulum_step beside a2c_point_step at the same B in the SAME process, the two alternating: GPU microseconds per env
    step of the post form at B = 32, 256, 2048, timed INSIDE a replayed hipGraph of 200 steps (50 replays between two HIP
    events), so that the figure is kernel time and not the rate at which the binding issues launches.  The Pendulum frame is
    some eighty 64-bit integer operations (two nested series); the Point frame a few dozen 32-bit ones;
  * ``--learn N``: a learning record -- ONE ``train()`` run of N epochs on "Pendulum-device" with ``eval_pool="device"`` and a
    fixed seed; the evaluation return after every epoch beside the return of the untrained net on the same kind of
    evaluation worlds (the first epoch's figure is taken after ONE update; ``untrained`` is measured before any) and the
    -1225 a uniform-random policy averaged in the prototype of the rules;
  * ``--norm``: the running-normalisation leg (hyps ``norm_obs`` / ``norm_rewards``) and nothing else: ms per
    epoch on the "device_graph" path with the keys off and with both on, the samples of the two alternating; GPU microseconds
    per a2c_vecnorm_step launch (both parts, B = 256, L = 4) inside a replayed hipGraph of 200 launches; with ``--learn N`` the
    learning record repeated with both keys on.  ``--out profiles/vecnorm_bench.json``;
  * ``--gauss-loss {reference,exact}``: the value of hyps ``gauss_loss`` in the epoch samples and in
    ``--learn``; ``--exact`` is the leg that sets the two beside each other and nothing else: ms per epoch on the
    "device_graph" path under "reference" and under "exact", the samples of the two alternating; with ``--learn N`` the
    learning record under "exact" (with ``--norm`` too: that record with both normalisation keys on).
    ``--out profiles/pendulum_exact_bench.json``;
  * ``--bootstrap-truncated``: the leg of hyps ``bootstrap_truncated`` and nothing else: ms per epoch of
    FCModel on the "device_graph" path with the key off and on, the samples of the two alternating (the key adds one N-row
    forward and three small launches to the update, and two stores per lane to the world step); with ``--learn N`` the
    learning record with the key on (``--gauss-loss`` and ``--norm`` as given).  ``--out profiles/pendulum_trunc_bench.json``;
  * ``--ppo-epochs K [--ppo-clip E]``: the leg of hyps ``ppo_epochs`` / ``ppo_clip`` and nothing else: ms
    per epoch of FCModel on the "device_graph" path with the keys absent and with ``ppo_epochs = K``, the samples of the two
    alternating (every further epoch of the update adds one forward, one loss launch, one backward and one optimiser step);
    with ``--learn N`` the learning record with the keys (``--gauss-loss``, ``--norm`` and ``--bootstrap-truncated`` as given;
    a Gaussian net needs ``--gauss-loss exact``).  ``--out profiles/ppo_bench.json``.

Method: ONE PROCESS PER SAMPLE.  ``--sample WHAT`` runs one sample in this process (a warm-up that allocates, tunes and
captures; then ``--epochs`` epochs, or the graph replays, between two HIP events) and prints one JSON line; without it the
tool starts ``--repeats`` such processes per figure, one after the other, and reports the median with min and max.

    python tools/pendulum_bench.py [--repeats 5] [--epochs 30] [--host-epochs 8] [--learn 300] [--only ...] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-a2c_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MODELS = ("FCModel", "GRUFCModel")
PATHS = ("device_graph", "device_eager", "host_serial", "host_process")
KERNEL_B = (32, 256, 2048)
WORLD = dict(max_episode_steps=200)
POINT_WORLD = dict(targets_to_win=3, max_episode_steps=1000)
UNIFORM_RANDOM = -1225.0          # 200 episodes of 200 frames under uniform(-2, 2) torques, the prototype of the rules
# the learning run: what train() gets beside its defaults
LEARN = dict(model="FCModel", env_type="Pendulum-device", eval_pool="device", n_envs=256, n_rollouts=256, n_tsteps=16,
             n_frame_stack=1, h_size=128, lr=1e-3, gamma=.95, lambda_=.95, entr_coef=.001, val_coef=.5, max_norm=.5,
             optim_type="RMSprop", n_test_eps=15, max_eval_steps=200, eval_chunk=40, seed=3, max_tsteps=1e12)


def event_ms(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


NORM_KEYS = dict(norm_obs=True, norm_rewards=True)


def ppo_keys(ppo):
    """ppo: (epochs, clip) or None (the keys absent)"""
    return dict(ppo_epochs=int(ppo[0]), ppo_clip=float(ppo[1])) if ppo else {}


def hyps_for(n_envs, T, path, norm=False, gauss_loss="reference", trunc=False, ppo=None):
    return dict(NORM_KEYS if norm else {}, **(dict(bootstrap_truncated=True) if trunc else {}), **ppo_keys(ppo), gauss_loss=gauss_loss, gamma=.99, lambda_=.98, n_tsteps=T, n_rollouts=n_envs, n_envs=n_envs, n_frame_stack=4, action_shift=0,
                render=False, env_type="Pendulum-device" if path.startswith("device") else "Pendulum-host", use_bptt=False,
                use_nstep_rets=False, norm_advs=True, entr_coef=.005, pi_coef=1.0, val_coef=.5, max_norm=.5, lr=1e-4,
                optim_type="RMSprop", is_discrete=False, h_size=256, seed=0, rollout_graphs=path != "device_eager")


def sample_vecnorm(B=256, L=4, C=4, T=16, launches=200, replays=50, rounds=3):
    """GPU microseconds per a2c_vecnorm_step (observations and rewards, update on): `launches` launches captured into one
    hipGraph, `replays` replays between two HIP events; the median of the rounds"""
    import torch
    from a2c_amd import ops
    from a2c_amd.vecnorm import DeviceVecNorm
    dv = DeviceVecNorm(L, B, .99)
    g = torch.Generator(device="cuda").manual_seed(3)
    out = torch.randn((B, C * L), device="cuda", generator=g)
    rewards, dones = torch.randn(B * T, device="cuda", generator=g), torch.zeros(B * T, device="cuda")

    def play():
        for i in range(launches):
            dv.launch(B, 0, out_ptr=out.data_ptr(), out_stride=C * L, C=C, rewards=rewards, dones=dones, T=T, t=i % T)
    play()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        play()
    for _ in range(3):
        graph.replay()
    us = [1e3 * event_ms(graph.replay, replays) / (launches * replays) for _ in range(rounds)]
    return dict(vecnorm_step=statistics.median(us))


def sample_epoch(model, path, n_envs, T, epochs, norm=False, gauss_loss="reference", trunc=False, ppo=None):
    import torch
    import a2c_amd
    from a2c_amd import preprocessing
    from a2c_amd.pendulum import DevicePendulumPool, PendulumEnv, PendulumFactory
    from a2c_amd.runner import HostEnvPool, Runner, SequentialEnvironment
    from a2c_amd.updater import Updater
    hyps = hyps_for(n_envs, T, path, norm, gauss_loss, trunc, ppo)
    torch.manual_seed(0)
    net = getattr(a2c_amd.models, model)([4, 4], 1, h_size=256, is_discrete=False)
    N = n_envs * T
    D = dict(states=torch.zeros(N, 4, 4, device="cuda"), deltas=torch.zeros(N, device="cuda"), rewards=torch.zeros(N, device="cuda"),
             dones=torch.zeros(N, device="cuda"), actions=torch.zeros(N, 1, device="cuda"))
    if net.is_recurrent:
        D["h_states"] = torch.zeros(N, net.h_size, device="cuda")
    if trunc:
        D.update(truncs=torch.zeros(N, device="cuda"), final_obs=torch.zeros(N, 4, device="cuda"))
    if path.startswith("device"):
        pool = DevicePendulumPool(n_envs, "cuda", seed=1, **WORLD)
    elif path == "host_serial":
        pool = HostEnvPool([PendulumEnv(seed=1, env_id=j, **WORLD) for j in range(n_envs)], frame_shape=(1, 4))
    else:
        from a2c_amd.hostpool import ProcessEnvPool
        kws = [dict(env_type="Pendulum-host", preprocessor=preprocessing.null_prep, seed=1,
                    env_fn=PendulumFactory(env_id=j, seed=1, **WORLD)) for j in range(n_envs)]
        pool = ProcessEnvPool(SequentialEnvironment, n_envs, env_kwargs=kws, n_workers=8, action_dim=1, frame_shape=(1, 4))
    r = Runner(D, hyps, None, None, None, env_pool=pool)
    upd = Updater(net, hyps)
    upd.vecnorm = lambda: r.vecnorm
    slots = list(range(n_envs))

    def epoch():
        r.rollout(net, slots, hyps)
        r.finish()
        upd.update_model(D)
    try:
        for _ in range(4):
            epoch()
        ms = event_ms(epoch, epochs)
    finally:
        r.close()
    return dict(ms_per_epoch=ms / epochs, env_steps_per_s=N * epochs / (ms * 1e-3))


def sample_kernel(B, steps=200, C=4, replays=50, rounds=3):
    """GPU microseconds per env step of the post forms of a2c_pendulum_step and a2c_point_step: `steps` steps captured into one
    hipGraph each (states ping-pong between two (B, C * HW) buffers), `replays` replays timed between two HIP events, the two
    worlds alternating `rounds` times; the median of the rounds"""
    import torch
    from a2c_amd import ops
    from a2c_amd.pendulum import DevicePendulumPool
    from a2c_amd.point import DevicePointPool
    g = torch.Generator(device="cuda").manual_seed(3)
    acts = dict(pendulum=(2.5 * torch.randn((64, B, 1), device="cuda", generator=g), 1),
                point=(1.5 * torch.randn((64, B, 2), device="cuda", generator=g), 2))
    graphs = {}
    for name in ("pendulum", "point"):
        pool = DevicePendulumPool(B, "cuda", seed=1, **WORLD) if name == "pendulum" else DevicePointPool(B, "cuda", seed=1, **POINT_WORLD)
        pool.reset_all()
        S = C * pool.HW
        x = [torch.zeros((B, S), device="cuda") for _ in range(2)]
        rewards, dones, deltas = (torch.zeros(2 * B, device="cuda") for _ in range(3))
        val, val_prev = torch.rand(B, device="cuda"), torch.zeros(B, device="cuda")
        a, stride = acts[name]

        def play(pool=pool, S=S, x=x, rewards=rewards, dones=dones, deltas=deltas, val=val, val_prev=val_prev, a=a, stride=stride):
            for i in range(steps):
                prev, nxt = x[i & 1].data_ptr(), x[1 - (i & 1)].data_ptr()
                post = ops.world_post(val.data_ptr(), 1, val_prev, rewards, dones, deltas, 2, 1, 0, .99, False, prev, S, nxt, S, C)
                pool.device_step_post(1, 0, B, (a[i & 63].data_ptr(), stride), post)
        play()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with ops.graph_capture(graph):
            play()
        for _ in range(3):
            graph.replay()
        graphs[name] = (graph, pool, x, rewards, dones, deltas, val, val_prev)      # (the buffers stay alive with the graph)
    us = {name: [] for name in graphs}
    for _ in range(rounds):
        for name in graphs:
            us[name].append(1e3 * event_ms(graphs[name][0].replay, replays) / (steps * replays))
    out = {name + "_step_post": statistics.median(v) for name, v in us.items()}
    out["pendulum_over_point"] = out["pendulum_step_post"] / out["point_step_post"]
    return out


def sample_learn(epochs, norm=False, gauss_loss="reference", trunc=False, ppo=None):
    """one train() run -> the evaluation return per epoch, and the untrained net's on worlds of the same kind (norm: with
    norm_obs and norm_rewards; the untrained net is then evaluated as every later epoch is, through a frozen block -- a fresh
    one, count 1e-4, mean 0, var 1, which is where train()'s own block starts)"""
    import time
    import torch
    import a2c_amd
    from a2c_amd.pendulum import DevicePendulumPool
    from a2c_amd.runner import DeviceStatsRunner
    from a2c_amd.training import DEFAULTS, train
    folder = tempfile.mkdtemp(prefix="pendulum_learn_")
    keys = dict(NORM_KEYS if norm else {}, **(dict(bootstrap_truncated=True) if trunc else {}), **ppo_keys(ppo), gauss_loss=gauss_loss)
    hyps = dict(LEARN, exp_name="pendulum_learn", main_path=folder, **keys)
    # the untrained net: train()'s own construction (same seed, same defaults), evaluated as train() evaluates
    full = dict(DEFAULTS, **hyps, is_discrete=False, action_shift=0, state_shape=[hyps["n_frame_stack"], 4], action_size=1)
    torch.manual_seed(hyps["seed"])
    net0 = getattr(a2c_amd.models, hyps["model"])(full["state_shape"], 1, bnorm=False,
                                                  **{k: v for k, v in full.items() if k != "use_bnorm"}).cuda()
    net0._ensure_device()
    fresh = None
    if norm:
        from a2c_amd.vecnorm import DeviceVecNorm
        fresh = DeviceVecNorm(4, hyps["n_envs"], full["gamma"])
    untrained = DeviceStatsRunner(full, DevicePendulumPool(hyps["n_test_eps"], "cuda", seed=hyps["seed"], **WORLD),
                                  norm=fresh).rollout(net0)
    curve = []

    class _Tap:
        """train() prints nothing we can read back per epoch: keep what its evaluator returned"""

        def __init__(self, inner):
            self.inner = inner

        def rollout(self, net):
            v = self.inner.rollout(net)
            curve.append(round(float(v), 3))
            return v
    import a2c_amd.training as tr
    real = tr.DeviceStatsRunner
    tr.DeviceStatsRunner = lambda *a, **k: _Tap(real(*a, **k))
    t0 = time.time()
    try:
        best = train(None, hyps, verbose=False, max_epochs=epochs)
    finally:
        tr.DeviceStatsRunner = real
    n = max(1, len(curve) // 10)
    return dict(settings=dict(LEARN, **keys), epochs=epochs, seconds=round(time.time() - t0, 1),
                env_steps=epochs * LEARN["n_envs"] * LEARN["n_tsteps"], untrained=round(float(untrained), 3),
                uniform_random=UNIFORM_RANDOM, best=round(float(best), 3), first_tenth_mean=round(statistics.mean(curve[:n]), 3),
                last_tenth_mean=round(statistics.mean(curve[-n:]), 3), eval_return_per_epoch=curve)


def spread(xs, nd=3):
    return dict(median=round(statistics.median(xs), nd), min=round(min(xs), nd), max=round(max(xs), nd), samples=[round(x, nd) for x in xs])


def child(args, what, gauss_loss=None, ppo=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--sample", what, "--epochs", str(args.epochs), "--host-epochs",
           str(args.host_epochs), "--n-envs", str(args.n_envs), "--n-tsteps", str(args.n_tsteps), "--gauss-loss",
           gauss_loss or args.gauss_loss]
    if ppo:
        cmd += ["--ppo-epochs", str(args.ppo_epochs), "--ppo-clip", str(args.ppo_clip)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=args.sample_timeout).stdout
    return json.loads(out.strip().splitlines()[-1])


def norm_leg(args):
    """keys off / both on, alternating samples of the device_graph path; the launch; optionally the learning record"""
    import torch
    res = {}
    if args.out and os.path.exists(args.out):      # records this leg does not produce (a comparison with a parent commit,
        with open(args.out) as f:                  # headline samples; an earlier learning record without --learn) stay
            res = json.load(f)
    res.update(device=torch.cuda.get_device_name(0), repeats=args.repeats, n_envs=args.n_envs, n_tsteps=args.n_tsteps,
               epochs=args.epochs, optim="RMSprop", world=WORLD, path="device_graph", ms_per_epoch={})
    for model in MODELS:
        rows = dict(keys_off=[], both_on=[])
        for _ in range(args.repeats):
            rows["keys_off"].append(child(args, f"epoch:{model}:device_graph")["ms_per_epoch"])
            rows["both_on"].append(child(args, f"epoch:{model}:device_graph:norm")["ms_per_epoch"])
        res["ms_per_epoch"][model] = {k: spread(v) for k, v in rows.items()}
        print(f"# {model}: {res['ms_per_epoch'][model]}", file=sys.stderr, flush=True)
    res["vecnorm_step_us"] = spread([child(args, "vecnorm")["vecnorm_step"] for _ in range(args.repeats)])
    print(f"# a2c_vecnorm_step: {res['vecnorm_step_us']} us", file=sys.stderr, flush=True)
    if args.learn > 0:
        res["learning_norm"] = child(args, f"learn:{args.learn}:norm")
        L = res["learning_norm"]
        print(f"# learning with both keys, {L['epochs']} epochs in {L['seconds']} s: untrained {L['untrained']}, first tenth "
              f"{L['first_tenth_mean']}, last tenth {L['last_tenth_mean']}, best {L['best']}", file=sys.stderr, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


def exact_leg(args):
    """gauss_loss "reference" / "exact", alternating samples of the device_graph path; optionally the learning record under
    "exact" (with --norm: with both normalisation keys on), kept under its own name beside what the file already holds"""
    import torch
    res = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res.update(device=torch.cuda.get_device_name(0), world=WORLD)

    def save():
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    if args.repeats > 0:            # (--repeats 0 --learn N: the learning record alone)
        res.update(repeats=args.repeats, n_envs=args.n_envs, n_tsteps=args.n_tsteps, epochs=args.epochs, optim="RMSprop",
                   path="device_graph", ms_per_epoch={})
        for model in MODELS:
            rows = dict(reference=[], exact=[])
            for _ in range(args.repeats):
                for mode in rows:
                    rows[mode].append(child(args, f"epoch:{model}:device_graph", mode)["ms_per_epoch"])
            res["ms_per_epoch"][model] = {k: spread(v) for k, v in rows.items()}
            print(f"# {model}: {res['ms_per_epoch'][model]}", file=sys.stderr, flush=True)
            save()
    if args.learn > 0:
        name = "learning_exact_norm" if args.norm else "learning_exact"
        L = res[name] = child(args, f"learn:{args.learn}" + (":norm" if args.norm else ""), "exact")
        print(f"# {name}, {L['epochs']} epochs in {L['seconds']} s: untrained {L['untrained']}, first tenth "
              f"{L['first_tenth_mean']}, last tenth {L['last_tenth_mean']}, best {L['best']}", file=sys.stderr, flush=True)
    save()
    print(json.dumps(res))


def trunc_leg(args):
    """hyps bootstrap_truncated off / on, alternating samples of FCModel on the device_graph path; optionally the learning
    record with the key on, kept under its own name beside what the file already holds (a parent commit's figure among it)"""
    import torch
    res = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res.update(device=torch.cuda.get_device_name(0), world=WORLD)

    def save():
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    tag = ":norm" if args.norm else ""
    if args.repeats > 0:            # (--repeats 0 --learn N: the learning record alone)
        res.update(repeats=args.repeats, n_envs=args.n_envs, n_tsteps=args.n_tsteps, epochs=args.epochs, optim="RMSprop",
                   path="device_graph", gauss_loss=args.gauss_loss, norm=bool(args.norm))
        rows = dict(key_off=[], key_on=[])
        for _ in range(args.repeats):
            rows["key_off"].append(child(args, f"epoch:FCModel:device_graph{tag}")["ms_per_epoch"])
            rows["key_on"].append(child(args, f"epoch:FCModel:device_graph{tag}:trunc")["ms_per_epoch"])
        res["ms_per_epoch"] = {"FCModel": {k: spread(v) for k, v in rows.items()}}
        print(f"# FCModel: {res['ms_per_epoch']['FCModel']}", file=sys.stderr, flush=True)
        save()
    if args.learn > 0:
        name = "learning" + ("_exact" if args.gauss_loss == "exact" else "") + ("_norm" if args.norm else "") + "_trunc"
        L = res[name] = child(args, f"learn:{args.learn}{tag}:trunc")
        print(f"# {name}, {L['epochs']} epochs in {L['seconds']} s: untrained {L['untrained']}, first tenth "
              f"{L['first_tenth_mean']}, last tenth {L['last_tenth_mean']}, best {L['best']}", file=sys.stderr, flush=True)
    save()
    print(json.dumps(res))


def ppo_leg(args):
    """hyps ppo_epochs / ppo_clip absent / given, alternating samples of FCModel on the device_graph path; optionally the
    learning record with the keys, each kept under a name that carries K beside what the file already holds"""
    import torch
    res = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res.update(device=torch.cuda.get_device_name(0), world=WORLD)

    def save():
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    tag = (":norm" if args.norm else "") + (":trunc" if args.bootstrap_truncated else "")
    K = args.ppo_epochs
    if args.repeats > 0:            # (--repeats 0 --learn N: the learning record alone)
        res.update(repeats=args.repeats, n_envs=args.n_envs, n_tsteps=args.n_tsteps, epochs=args.epochs, optim="RMSprop",
                   path="device_graph", gauss_loss=args.gauss_loss, norm=bool(args.norm), trunc=bool(args.bootstrap_truncated),
                   ppo_clip=args.ppo_clip)
        rows = {f"keys_absent_beside_{K}": [], f"ppo_epochs_{K}": []}
        for _ in range(args.repeats):
            rows[f"keys_absent_beside_{K}"].append(child(args, f"epoch:FCModel:device_graph{tag}")["ms_per_epoch"])
            rows[f"ppo_epochs_{K}"].append(child(args, f"epoch:FCModel:device_graph{tag}", ppo=True)["ms_per_epoch"])
        res.setdefault("ms_per_epoch", {}).setdefault("FCModel", {}).update({k: spread(v) for k, v in rows.items()})
        print(f"# FCModel: { {k: res['ms_per_epoch']['FCModel'][k] for k in rows} }", file=sys.stderr, flush=True)
        save()
    if args.learn > 0:
        name = ("learning" + ("_exact" if args.gauss_loss == "exact" else "") + ("_norm" if args.norm else "")
                + ("_trunc" if args.bootstrap_truncated else "") + f"_ppo{K}")
        L = res[name] = child(args, f"learn:{args.learn}{tag}", ppo=True)
        print(f"# {name}, {L['epochs']} epochs in {L['seconds']} s: untrained {L['untrained']}, first tenth "
              f"{L['first_tenth_mean']}, last tenth {L['last_tenth_mean']}, best {L['best']}", file=sys.stderr, flush=True)
    save()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5, help="samples per figure: one process each")
    ap.add_argument("--epochs", type=int, default=30, help="epochs per sample on the device paths")
    ap.add_argument("--host-epochs", type=int, default=8, help="epochs per sample on the host paths")
    ap.add_argument("--n-envs", type=int, default=256)
    ap.add_argument("--n-tsteps", type=int, default=16)
    ap.add_argument("--learn", type=int, default=0, help="epochs of the learning record (0: none)")
    ap.add_argument("--only", default=None, help="comma-separated subset of: kernel, learn, " + ", ".join(PATHS))
    ap.add_argument("--norm", action="store_true", help="the running-normalisation leg only (see the module docstring)")
    ap.add_argument("--gauss-loss", default="reference", choices=("reference", "exact"),
                    help="hyps['gauss_loss'] of the epoch samples and of --learn")
    ap.add_argument("--exact", action="store_true", help="the gauss_loss leg only (see the module docstring)")
    ap.add_argument("--bootstrap-truncated", action="store_true",
                    help="the bootstrap_truncated leg only (see the module docstring)")
    ap.add_argument("--ppo-epochs", type=int, default=0,
                    help="hyps['ppo_epochs'] (0: the keys absent); without --sample: the ppo leg only (see the module docstring)")
    ap.add_argument("--ppo-clip", type=float, default=0.2, help="hyps['ppo_clip'] beside --ppo-epochs")
    ap.add_argument("--sample", default=None, help="run ONE sample in this process: kernel:B, vecnorm, "
                                                   "epoch:MODEL:PATH[:norm][:trunc] or learn:N[:norm][:trunc]")
    ap.add_argument("--sample-timeout", type=float, default=600.0)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "pendulum_bench needs the MI355X"
    ppo = (args.ppo_epochs, args.ppo_clip) if args.ppo_epochs else None
    if args.sample:
        kind, *rest = args.sample.split(":")
        if kind == "kernel":
            res = sample_kernel(int(rest[0]))
        elif kind == "vecnorm":
            res = sample_vecnorm()
        elif kind == "learn":
            res = sample_learn(int(rest[0]), norm="norm" in rest[1:], gauss_loss=args.gauss_loss, trunc="trunc" in rest[1:],
                               ppo=ppo)
        else:
            model, path = rest[:2]
            res = sample_epoch(model, path, args.n_envs, args.n_tsteps, args.epochs if path.startswith("device") else args.host_epochs,
                               norm="norm" in rest[2:], gauss_loss=args.gauss_loss, trunc="trunc" in rest[2:], ppo=ppo)
        print(json.dumps(res))
        return
    if ppo:
        return ppo_leg(args)
    if args.bootstrap_truncated:
        return trunc_leg(args)
    if args.exact:
        return exact_leg(args)
    if args.norm:
        return norm_leg(args)
    only = set(args.only.split(",")) if args.only else {"kernel", "learn", *PATHS}
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, n_envs=args.n_envs, n_tsteps=args.n_tsteps,
               epochs=args.epochs, host_epochs=args.host_epochs, optim="RMSprop", gauss_loss=args.gauss_loss, world=WORLD,
               point_world=POINT_WORLD, epoch={},
               kernel_us_per_env_step={})
    if args.out and os.path.exists(args.out):      # a run with --only adds to what an earlier run measured
        with open(args.out) as f:
            old = json.load(f)
        for k in ("epoch", "kernel_us_per_env_step", "learning"):
            if k in old:
                res[k] = old[k]

    def save():
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    if "kernel" in only:
        for B in KERNEL_B:
            rows = [child(args, f"kernel:{B}") for _ in range(args.repeats)]
            res["kernel_us_per_env_step"][f"B{B}"] = {k: spread([r[k] for r in rows]) for k in rows[0]}
            print(f"# kernel B={B}: {res['kernel_us_per_env_step'][f'B{B}']}", file=sys.stderr, flush=True)
            save()
    for model in MODELS:
        for path in PATHS:
            if path not in only:
                continue
            rows = [child(args, f"epoch:{model}:{path}") for _ in range(args.repeats)]
            res["epoch"].setdefault(model, {})[path] = dict(ms_per_epoch=spread([r["ms_per_epoch"] for r in rows]),
                                                            env_steps_per_s=spread([r["env_steps_per_s"] for r in rows], 0))
            print(f"# {model} {path}: {res['epoch'][model][path]['ms_per_epoch']}", file=sys.stderr, flush=True)
            save()
    if "learn" in only and args.learn > 0:
        res["learning"] = child(args, f"learn:{args.learn}")
        L = res["learning"]
        print(f"# learning, {L['epochs']} epochs in {L['seconds']} s: untrained {L['untrained']}, first tenth {L['first_tenth_mean']}, "
              f"last tenth {L['last_tenth_mean']}, best {L['best']}", file=sys.stderr, flush=True)
        save()
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
