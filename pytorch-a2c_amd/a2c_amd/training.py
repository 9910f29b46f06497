"""Epoch driver with the reference's protocol (a2c/training.py:23-238) around the MI355X engine
(SURVEY.md section 8, row f1).  Same hyper-parameter keys as training_scripts/hyperparams.json; same
files in the save folder (``net.p``, ``best_net.p``, ``optim.p``, ``log.txt``); same loop:
wait for ``n_rollouts`` tokens on ``stop_q`` -> ``updater.update_model(shared_data)`` -> evaluation
rollout -> re-open the gate -> every 10 epochs save.

Differences forced by the design: ONE ``Runner`` (in a thread of this process) drives all
``n_envs`` envs in lock-step; the envs themselves are stepped by worker PROCESSES behind the pinned
pool region (``hostpool.ProcessEnvPool``, the counterpart of the reference's ``n_envs`` runner
processes, training.py:109-121), and runner and updater share the net object, so the weight publish
``net.load_state_dict(updater.net.state_dict())`` (training.py:165) disappears.  A failure inside
the runner thread or an env worker is re-raised here instead of dead-locking ``stop_q.get()``.  ``ml_utils`` (hyper-search CLI, un-vendored in the reference) is
not mirrored; the two helpers the loop needs (experiment numbering / save folder) are restated.
"""
import os
import queue
import threading
import time
from collections import deque

import numpy as np
import torch

from . import models, preprocessing, vecnorm
from .families import DEVICE_TYPES, FAMILIES, VECTOR_WORLDS, family_of
from .runner import (DeviceStatsRunner, HostEnvPool, Runner, SequentialEnvironment, StatsRunner,
                     check_bootstrap_truncated, gym_env_pool)
from .updater import Updater, gauss_loss_mode, ppo_refusal, ppo_settings
from .worlds import TRAINING_ONLY
from .utils import cuda_if, deque_maxmin, try_key

DEFAULTS = dict(n_frame_stack=4, n_rollouts=None, n_past_rews=25, h_size=256, lr=1e-4, lr_low=1e-12, lambda_=.98,
                gamma=.99, gamma_high=.995, val_coef=.5, entr_coef=.005, entr_coef_low=.001, pi_coef=1.0, max_norm=.5,
                resume=False, render=False, decay_lr=False, decay_entr=False, use_nstep_rets=False, norm_advs=True,
                use_bnorm=False, use_bptt=False, optim_type="RMSprop", n_test_eps=15, max_tsteps=4e7,
                gauss_loss="reference", bootstrap_truncated=False, ppo_epochs=1, ppo_clip=0.2)


def get_exp_num(main_path, exp_name):
    """next free experiment number under main_path/exp_name (ml_utils.training.get_exp_num restated)"""
    folder = os.path.join(main_path, exp_name)
    nums = [int(d.rsplit("_", 1)[-1]) for d in (os.listdir(folder) if os.path.isdir(folder) else [])
            if d.rsplit("_", 1)[-1].isdigit()]
    return max(nums) + 1 if nums else 0


def get_save_folder(hyps):
    folder = os.path.join(hyps["main_path"], hyps["exp_name"], f"{hyps['exp_name']}_{hyps['exp_num']}")
    os.makedirs(folder, exist_ok=True)
    return folder


# The device-world families of train(), env_type "<family>-device" / "<family>-host": the records of families.py, one per
# world module (worlds.WorldFamily).  Nothing below names a family.
_WORLDS, _VECTOR_WORLDS = FAMILIES, VECTOR_WORLDS


def _world_family(env_type):
    """"Pong" of "Pong-device" / "Pong-host"; None for every other env_type"""
    fam = family_of(env_type)
    return None if fam is None else fam.name


def _norm_tensors(sd):
    """a RunningNorm state_dict with its float64 arrays as torch tensors: what norm.p / best_norm.p hold"""
    return {k: (torch.from_numpy(np.array(v, dtype=np.float64)) if isinstance(v, np.ndarray) else v) for k, v in sd.items()}


class _PositionalFactory:
    """env worker processes build env j as ``env_fn(j)`` whatever the callable names its parameter (the pool calls
    factories with keyword arguments)"""

    def __init__(self, fn):
        self.fn = fn

    def __call__(self, j):
        return self.fn(j)


def _complete_hyps(hyps, env_fn, eval_env):
    """``hyps`` over DEFAULTS, refused (a ValueError naming the key) or completed BEFORE anything is written or allocated ->
    (hyps, the record of the env_type's world family or None, the family's rules, the normaliser's settings or None)"""
    hyps = dict(DEFAULTS, **hyps)
    # gauss_loss: a value that is neither "reference" nor "exact", and "exact" where the action space is
    # known to be discrete (a device world's family, an env_fn's is_discrete key; a gym env's space is only known from the
    # probe, where the Updater refuses it)
    fam = family_of(hyps.get("env_type")) if env_fn is None else None
    discrete = ((not fam.float_actions) if fam is not None else
                (bool(try_key(hyps, "is_discrete", True)) if env_fn is not None else None))
    gauss_loss_mode(hyps, discrete)
    # ppo_epochs / ppo_clip: bad values, and for ppo_epochs >= 2 what hyps already tells -- a net other
    # than FCModel / GRUFCModel, a continuous action space under the reference's Gaussian loss; the Updater refuses the rest
    model = hyps.get("model")
    why = ppo_refusal(ppo_settings(hyps)[0], model if isinstance(model, str) else None, discrete, hyps["gauss_loss"])
    if why is not None:
        raise ValueError(why)
    # bootstrap_truncated: everything but the lane worlds' device pools under FCModel
    if try_key(hyps, "bootstrap_truncated", False):
        if env_fn is not None:
            raise ValueError("a2c_amd: bootstrap_truncated bootstraps time-limit episode ends of the lane worlds' device pools, "
                             "not an env_fn's envs")
        check_bootstrap_truncated(hyps)
    eval_pool = try_key(hyps, "eval_pool", None) or "host"
    if eval_pool not in ("host", "device"):
        raise ValueError(f"a2c_amd: hyps['eval_pool'] is 'host' or 'device', not {eval_pool!r}")
    if eval_pool == "device" and (eval_env is not None or env_fn is not None or hyps.get("env_type") not in DEVICE_TYPES):
        raise ValueError("a2c_amd: hyps['eval_pool'] = 'device' evaluates the device worlds (env_type "
                         f"{', '.join(map(repr, DEVICE_TYPES[:-1]))} or {DEVICE_TYPES[-1]!r}) and takes no eval_env / env_fn")
    # running normalisation: the device pools of the vector worlds, evaluated on lock-step twins or on
    # the device, and nothing else
    norm = vecnorm.norm_settings(hyps)
    if norm is not None:
        key, nfam = vecnorm.norm_key(hyps), family_of(hyps.get("env_type"))
        if env_fn is not None or nfam is None or not nfam.vector or hyps["env_type"] != nfam.name + "-device":
            raise ValueError(f"a2c_amd: {key} normalises inside the rollout slot of a device pool of the vector worlds "
                             f"(env_type {', '.join(repr(f + '-device') for f in VECTOR_WORLDS)}), not "
                             f"{hyps.get('env_type')!r}" + (" with an env_fn" if env_fn is not None else ""))
        if eval_env is not None:
            raise ValueError(f"a2c_amd: {key} evaluates on lock-step host twins (eval_pool='host') or on the device "
                             "(eval_pool='device'); a single eval_env plays the reference's serial loop, which is not normalised")
    # the family's own refusals: keys it does not take or that are out of bounds, a net or an env pool that cannot play it
    rules = fam.check_hyps(hyps, hyps["env_type"] == fam.name + "-host") if fam is not None else None
    if hyps["n_rollouts"] is None:
        hyps["n_rollouts"] = hyps["n_envs"]
    hyps["main_path"] = try_key(hyps, "main_path", "./")
    return hyps, fam, rules, norm


def _build_envs(hyps, fam, rules, env_fn, eval_env):
    """the training env pool -- the device pool of the world family ``fam`` or its host twins behind a host pool, else the gym
    envs of ``env_type``, else ``env_fn``'s envs -- and the environment keys of the hyps that Runner, Updater and the nets read
    (prep_fxn, preprocessor, is_discrete, max_eval_steps, state_shape, action_size, action_shift) -> (pool, make_eval):
    ``make_eval(uniform_fn, eval_norm)`` builds the evaluation runner (None: none) once the Runner exists"""
    n_envs, seed = hyps["n_envs"], hyps["seed"]
    serial = try_key(hyps, "env_pool", "process") == "serial"
    raw = False
    if fam is not None:
        host = hyps["env_type"] == fam.name + "-host"
        world = dict(zip((k for k, _ in fam.world_keys), fam.world_from_hyps(hyps)), seed=seed)
        # device_prep: the workers hand on the RAW frames (null_prep) and a2c_frame_prep_u8 crops / strides them
        raw = fam.raw_frames(hyps, host, serial)
        hyps["prep_fxn"] = "null_prep" if raw else fam.prep
        prep = hyps["preprocessor"] = getattr(preprocessing, hyps["prep_fxn"])
        hyps["is_discrete"], n_act = not fam.float_actions, fam.n_act
        if fam.float_actions:      # a Box: in this process unless env_pool='process_f32' (as below for every continuous env)
            serial = try_key(hyps, "env_pool", None) != "process_f32"
        # a policy that circles never ends its evaluation episode: cap it (StatsRunner reads the key)
        hyps["max_eval_steps"] = try_key(hyps, "max_eval_steps", 2000)
        if fam.repeats:
            world.update(zip(("frame_skip", "sticky_num", "sticky_den"), fam.repeat_from_hyps(hyps)))
        # evaluation plays whole games for the game's score: the dynamics (frame_skip_max), not the training flags
        eval_world = dict(world, **{k: v for k, v in rules.items() if k not in TRAINING_ONLY})
        world.update(rules)
        mk_env = lambda j, kw=world: SequentialEnvironment(hyps["env_type"], getattr(preprocessing, fam.prep), seed=seed,
                                                           env_fn=fam.factory(env_id=j, **kw))
        world_shape = fam.frame_shape(world)
        if not host:
            pool = fam.pool(n_envs, device=cuda_if(torch.zeros(1)).device, **world)
        elif serial:
            pool = HostEnvPool([mk_env(j) for j in range(n_envs)], frame_shape=world_shape)
        else:
            from .hostpool import ProcessEnvPool
            kws = [dict(env_type=hyps["env_type"], preprocessor=prep, seed=seed, env_fn=fam.factory(env_id=j, **world))
                   for j in range(n_envs)]
            # frame_bits: {0, 1} uint8 planes cross the host link one bit per pixel; grey levels one byte per pixel
            pool = ProcessEnvPool(SequentialEnvironment, n_envs, env_kwargs=kws, n_workers=try_key(hyps, "n_env_workers", None),
                                  pong=fam.pong_done, action_shift=try_key(hyps, "action_shift", 0), frame_bits=fam.frame_bits,
                                  action_dim=n_act if fam.float_actions else None,
                                  # (null_prep puts an axis in front of a twin's (1, L) row: the states are the device pool's)
                                  frame_shape=world_shape if fam.vector else None)
    elif env_fn is None:
        hyps["preprocessor"] = getattr(preprocessing, hyps["prep_fxn"])
        probe = eval_env or SequentialEnvironment(**hyps)             # the probe for shapes (training.py:60-65)
        hyps["is_discrete"], n_act = probe.is_discrete, probe.n
    else:
        hyps["is_discrete"] = bool(try_key(hyps, "is_discrete", True))
    if not hyps["is_discrete"]:
        # float actions do not fit the process pool's int32 command words: continuous envs step in this process
        if "env_pool" in hyps and hyps["env_pool"] == "process":
            raise ValueError("a2c_amd: continuous action spaces need env_pool='serial' (the process env pool carries "
                             "int32 actions)")
        # ... unless asked for: env_pool='process_f32' = worker processes behind a pool with float action granules
        serial = try_key(hyps, "env_pool", None) != "process_f32"
    elif try_key(hyps, "env_pool", None) == "process_f32":
        raise ValueError("a2c_amd: env_pool='process_f32' carries float action vectors: it needs a continuous action space "
                         "(discrete envs use env_pool='process')")
    # float action granules per env (ProcessEnvPool(action_dim=n)); None = the int32 command-word pool
    f32_dim = None
    if not hyps["is_discrete"] and not serial:
        f32_dim = int(n_act if env_fn is None else hyps["action_size"])
    pong_v0 = hyps["env_type"] == "Pong-v0"                           # training.py:67-69: three actions from 1 on
    shift = 1 if pong_v0 else try_key(hyps, "action_shift", 0)
    if fam is not None:
        pass
    elif env_fn is None:
        pool = gym_env_pool(hyps, n_envs, seed, serial, action_shift=shift, rew_ema0=-1.0, action_dim=f32_dim)
    else:
        if serial:
            pool = HostEnvPool([env_fn(j) for j in range(n_envs)])
        else:
            from .hostpool import ProcessEnvPool
            pool = ProcessEnvPool(_PositionalFactory(env_fn), n_envs, env_kwargs=[dict(j=j) for j in range(n_envs)],
                                  n_workers=try_key(hyps, "n_env_workers", None), pong="Pong" in hyps["env_type"],
                                  action_shift=shift, probe_reset=True, frame_bits=bool(try_key(hyps, "frame_bits", False)),
                                  action_dim=f32_dim)
        n_act = hyps["action_size"]
    # (a pool that carries raw frames: the states are what the device makes of them)
    hyps["state_shape"] = [hyps["n_frame_stack"]] + list((world_shape if raw else pool.frame_shape)[1:])
    hyps["action_size"], hyps["action_shift"] = (3 if pong_v0 else n_act), shift
    n_eval = try_key(hyps, "n_test_eps", 15)

    def make_eval(uniform_fn, eval_norm):
        if (try_key(hyps, "eval_pool", None) or "host") == "device":
            # a second pool of the training pool's kind: same world and seed, n_test_eps worlds (DeviceStatsRunner gives them
            # the env ids of the host twins below, and fresh ones on every later call)
            return DeviceStatsRunner(hyps, type(pool)(n_eval, device=pool.device, **eval_world), uniform_fn=uniform_fn,
                                     norm=eval_norm)
        if eval_env is not None:                                      # the caller's single env (reference loop)
            return StatsRunner(hyps, env=eval_env)
        if fam is not None:
            # host twins of worlds the training pool does not play (env ids from 10007 on)
            return StatsRunner(hyps, envs=[mk_env(10007 + j, eval_world) for j in range(n_eval)], norm=eval_norm)
        return StatsRunner(hyps) if env_fn is None else None          # n_test_eps gym envs in lock-step on the device
    return pool, make_eval


def _rollout_buffers(hyps, net, shared_len, frame_shape):
    """the ``shared_data`` of the reference (training.py:88-101), device resident"""
    shared_data = {"states": cuda_if(torch.zeros((shared_len, *hyps["state_shape"]))),
                   "deltas": cuda_if(torch.zeros(shared_len)), "rewards": cuda_if(torch.zeros(shared_len)),
                   # (the reference keeps `actions` on the host, training.py:90,97; device resident here so that the
                   # rollout's device relay can write it -- nothing outside train() sees the dict)
                   # (continuous actions: one float row of n per sample, training.py:89-92)
                   "actions": cuda_if(torch.zeros(shared_len).long() if hyps["is_discrete"] else
                                      torch.zeros((shared_len, hyps["action_size"]))),
                   "dones": cuda_if(torch.zeros(shared_len))}
    if net.is_recurrent:
        shared_data["h_states"] = cuda_if(torch.zeros(shared_len, net.h_size))
    if try_key(hyps, "bootstrap_truncated", False):      # (section 6o: indexed like rewards; one observation per row)
        shared_data["truncs"] = cuda_if(torch.zeros(shared_len))
        shared_data["final_obs"] = cuda_if(torch.zeros((shared_len, int(np.prod(frame_shape)))))
    return shared_data


def train(_, hyps, verbose=True, env_fn=None, eval_env=None, max_epochs=None, uniform_fn=None, on_epoch=None):
    """``hyps``: the reference's flat dict (training_scripts/hyperparams.json; ``n_rollouts`` need not be a multiple of
    ``n_envs``).  ``env_fn(j)`` (optional) builds env j as an object with ``reset()/step(a)`` returning already
    prepped frames -- otherwise gym envs are made from ``env_type`` / ``prep_fxn`` like the reference.  With the
    default process env pool ``env_fn`` travels to the worker processes pickled: lambdas and closures need
    ``cloudpickle`` (else pass a module-level callable, or ``hyps['env_pool'] = 'serial'``).  ``uniform_fn`` /
    ``on_epoch(epoch, updater, shared_data)`` are test hooks (sampler uniforms; called after every update).
    Continuous (``Box``) envs step in this process unless ``hyps['env_pool'] = 'process_f32'``: worker processes behind a
    pool that carries float action vectors (``ProcessEnvPool(action_dim=n)``); ``'process'`` stays the int32 pool.
    The world families (families.py) need no gym: ``env_type`` "<family>-device" plays ``n_envs`` worlds
    in device memory (the family's ``Device<family>Pool``), "<family>-host" its host twins behind the usual ``env_pool``
    choices with the family's ``prep_fxn``; both are evaluated on host twins.  ``action_shift`` is 0 unless given.  A key or a
    net the family does not take is a ValueError before anything is written or allocated.  Keys, preprocessor, actions, nets
    and pools of each family are in its module's docstring:
      "Snake-device" / "Snake-host"          a2c_amd/snake.py
      "Pong-device" / "Pong-host"            a2c_amd/pong.py
      "Breakout-device" / "Breakout-host"    a2c_amd/breakout.py
      "Point-device" / "Point-host"          a2c_amd/point.py
      "CartPole-device" / "CartPole-host"    a2c_amd/cartpole.py ("CartPole-v1" stays gym's)
      "Pendulum-device" / "Pendulum-host"    a2c_amd/pendulum.py ("Pendulum-v1" stays gym's)
    ``hyps["eval_pool"] = "device"`` (the six ``*-device`` env types, no ``eval_env``) evaluates on the device instead: a
    second pool of ``n_test_eps`` worlds behind a ``DeviceStatsRunner`` (keys ``eval_chunk``, ``max_eval_steps``); the default
    ``"host"`` is the host twins.
    ``hyps["norm_obs"]`` / ``hyps["norm_rewards"]`` (``norm_clip_obs`` 10, ``norm_clip_rew`` 10,
    ``norm_eps`` 1e-8; ``gamma`` is the run's): running normalisation of the observations and of the rewards, baselines'
    VecNormalize, as one launch behind every env step of the slot -- "Point-device", "CartPole-device" and "Pendulum-device"
    only (anything else is a ValueError naming the key, before anything is written).  Evaluation normalises its observations
    by the training block as it stands and never its rewards; ``norm.p`` is written wherever ``optim.p`` is (and read on
    ``resume``), ``best_norm.p`` beside ``best_net.p``.
    ``hyps["gauss_loss"]``: ``"reference"`` (the default: the reference's Gaussian loss, at parity) or
    ``"exact"`` (the per-sample Gaussian log-likelihood loss with an entropy bonus, one launch per update), for continuous
    action spaces only (anything else is a ValueError naming the key); it changes the update alone, not the rollout, the
    sampling or the evaluation.
    ``hyps["bootstrap_truncated"]`` (default False: everything as it was): an episode that ends by
    ``max_episode_steps`` alone is cut short, not lost, so the targets of its closing step use r + gamma * V(the state it ended
    in) instead of r.  The lane worlds' step reports that state (a2c_<world>_step_trunc into ``truncs`` / ``final_obs`` of the
    rollout buffer) and the update adds gamma * V of it to the step's reward and delta before the scan.  "Point-device",
    "CartPole-device" and "Pendulum-device" with FCModel only (anything else -- GRUFCModel, the picture worlds, the ``-host``
    env types, gym envs, an ``env_fn`` -- is a ValueError naming the key, before anything is written); evaluation is untouched.
    ``hyps["ppo_epochs"]`` = K (int >= 1; default 1: everything as it was) and ``hyps["ppo_clip"]``
    (float > 0, default 0.2): with K >= 2 every rollout is used for K gradient steps on the same rows, advantages and
    returns instead of one -- the first the plain policy-gradient step, which also records every row's log-probability, the
    later ones under PPO's clipped-ratio objective against it (one whole-batch step per epoch: no minibatches, no value
    clipping, no KL early stopping); ``info`` gains ``ClipFrac`` and ``ApproxKL`` of the last epoch.  FCModel and GRUFCModel,
    discrete actions or Gaussian ones under ``gauss_loss="exact"``, one GPU (anything else is a ValueError naming the key);
    the rollout, the worlds and the evaluation are untouched.
    Returns the best evaluation reward."""
    hyps, fam, rules, norm = _complete_hyps(hyps, env_fn, eval_env)
    hyps["exp_num"] = get_exp_num(hyps["main_path"], hyps["exp_name"])
    save_folder = hyps["save_folder"] = get_save_folder(hyps)
    hyps["seed"] = try_key(hyps, "seed", int(time.time()))
    torch.manual_seed(hyps["seed"])
    np.random.seed(hyps["seed"])
    net_save_file, best_net_file = os.path.join(save_folder, "net.p"), os.path.join(save_folder, "best_net.p")
    optim_save_file, log_file = os.path.join(save_folder, "optim.p"), os.path.join(save_folder, "log.txt")
    # the normaliser's moments travel with the weights trained under them: norm.p beside optim.p, best_norm.p beside best_net.p
    norm_save_file, best_norm_file = os.path.join(save_folder, "norm.p"), os.path.join(save_folder, "best_norm.p")
    log = open(log_file, "a" if hyps["resume"] else "w")
    for k in sorted(hyps):
        log.write(k + ":" + str(hyps[k]) + "\n")
    pool, make_eval = _build_envs(hyps, fam, rules, env_fn, eval_env)
    action_size, shared_len = hyps["action_size"], hyps["n_tsteps"] * hyps["n_rollouts"]
    if verbose:
        print("State Shape:,", hyps["state_shape"], "Num Samples Per Update:", shared_len)

    net = getattr(models, hyps["model"])(hyps["state_shape"], action_size, bnorm=hyps["use_bnorm"],
                                         **{k: v for k, v in hyps.items() if k not in ("use_bnorm",)})
    if hyps["resume"]:
        net.load_state_dict(torch.load(net_save_file))
    net = cuda_if(net)
    net._ensure_device()            # the flat parameter arena exists BEFORE the runner thread and the Updater touch it
    shared_data = _rollout_buffers(hyps, net, shared_len, pool.frame_shape)
    n_rollouts = hyps["n_rollouts"]
    gate_q, stop_q, reward_q = queue.Queue(n_rollouts), queue.Queue(n_rollouts), queue.Queue(1)
    reward_q.put(-1)
    runner = Runner(shared_data, hyps, gate_q, stop_q, reward_q, env_pool=pool, uniform_fn=uniform_fn)
    if norm is not None and hyps["resume"]:
        runner.norm_state = torch.load(norm_save_file)
    # (the block is made by the rollout thread's start(): evaluation asks for it when it first runs, an epoch later)
    eval_norm = (lambda: runner.vecnorm) if norm is not None and norm["obs"] else None
    norm_sd = None
    thread = threading.Thread(target=runner.run, args=(net,), daemon=True)
    thread.start()

    def collect():
        """stop_q.get() that notices a dead runner: a None token or a stopped thread re-raises its exception"""
        while True:
            try:
                tok = stop_q.get(timeout=1.0)
            except queue.Empty:
                if not thread.is_alive():
                    raise RuntimeError("the rollout thread stopped") from runner.error
                continue
            if tok is None:
                raise RuntimeError("the rollout thread failed") from runner.error
            return tok
    updater = Updater(net, hyps)
    updater.vecnorm = eval_norm      # (bootstrap_truncated under norm_obs: the final states pass through the Runner's block)
    if hyps["resume"]:
        updater.optim.load_state_dict(torch.load(optim_save_file))
    for i in range(n_rollouts):
        gate_q.put(i)
    stats_runner = make_eval(uniform_fn, eval_norm)
    entr_coef_diff, lr_diff = hyps["entr_coef"] - hyps["entr_coef_low"], hyps["lr"] - hyps["lr_low"]
    past_rews = deque([0] * hyps["n_past_rews"])
    best_eval_rew, epoch, T = -np.inf, 0, 0
    while T < hyps["max_tsteps"] and (max_epochs is None or epoch < max_epochs):
        basetime = time.time()
        epoch += 1
        for _i in range(n_rollouts):                                   # barrier: all slots collected
            collect()
        T += shared_len
        avg_reward = reward_q.get()
        reward_q.put(avg_reward)
        updater.update_model(shared_data)
        if on_epoch is not None:
            on_epoch(epoch, updater, shared_data)
        eval_rew = stats_runner.rollout(net) if stats_runner is not None else avg_reward
        if norm is not None:
            # the moments as the collected rollouts left them (the rollout thread is idle until the gate re-opens): what this
            # epoch's saves write; one device read
            norm_sd = _norm_tensors(runner.vecnorm.state_dict())
        if eval_rew > best_eval_rew:
            best_eval_rew = eval_rew
            updater.save_model(best_net_file, None)
            if norm_sd is not None:
                torch.save(norm_sd, best_norm_file)
        for i in range(n_rollouts):                                    # resume data collection
            gate_q.put(i)
        if hyps["decay_lr"]:
            updater.new_lr(max((1 - T / hyps["max_tsteps"]), 0) * lr_diff + hyps["lr_low"])
        if hyps["decay_entr"]:
            updater.entr_coef = entr_coef_diff * max((1 - T / hyps["max_tsteps"]), 0) + hyps["entr_coef_low"]
        if epoch % 10 == 0:
            updater.save_model(net_save_file, optim_save_file)
            if norm_sd is not None:
                torch.save(norm_sd, norm_save_file)
        past_rews.popleft()
        past_rews.append(avg_reward)
        max_rew, min_rew = deque_maxmin(past_rews)
        avg_action = shared_data["actions"].float().mean().item()
        if verbose:
            print("Epoch {} - T: {} -- {}".format(epoch, T, save_folder))
            updater.print_statistics()
        updater.log_statistics(log, T, avg_reward, avg_action, best_eval_rew)
        log.write("Grad Norm: {:.5f} – Avg Action: {:.5f} - Best EvalRew: {:.5f}\nPast Rews – High: {:.5f} - Low: {:.5f}\n"
                  "Time: {}\n\n".format(float(updater.norm), avg_action, best_eval_rew, max_rew, min_rew,
                                        time.time() - basetime))
    updater.save_model(net_save_file, optim_save_file)
    if norm_sd is not None:
        torch.save(norm_sd, norm_save_file)
    log.write("\nBestRew:" + str(best_eval_rew))
    log.close()
    for _i in range(n_rollouts):        # let the rollout the loop re-opened finish, then stop the thread and the env workers
        collect()
    gate_q.put(None)
    thread.join(timeout=30)
    runner.close()
    return best_eval_rew
