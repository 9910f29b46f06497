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

from . import breakout, cartpole, models, pendulum, point, pong, preprocessing, snake, vecnorm, worlds
from .runner import (DeviceStatsRunner, HostEnvPool, Runner, SequentialEnvironment, StatsRunner,
                     check_bootstrap_truncated)
from .updater import Updater, gauss_loss_mode
from .utils import cuda_if, deque_maxmin, try_key

DEFAULTS = dict(n_frame_stack=4, n_rollouts=None, n_past_rews=25, h_size=256, lr=1e-4, lr_low=1e-12, lambda_=.98,
                gamma=.99, gamma_high=.995, val_coef=.5, entr_coef=.005, entr_coef_low=.001, pi_coef=1.0, max_norm=.5,
                resume=False, render=False, decay_lr=False, decay_entr=False, use_nstep_rets=False, norm_advs=True,
                use_bnorm=False, use_bptt=False, optim_type="RMSprop", n_test_eps=15, max_tsteps=4e7,
                gauss_loss="reference", bootstrap_truncated=False)


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


# The device-world families of train(), env_type "<family>-device" / "<family>-host": the module of a2c_amd, its preprocessor,
# the "Pong" done override, the one-bit frame transport of the process pool ({0, 1} frames only), the names of what the
# module's world_from_hyps returns (the world kwargs), whether the family takes frame_skip / sticky_num / sticky_den, and which
# of frame_skip_max / episodic_life / clip_rewards it takes.
_WORLDS = {
    "Snake": (snake, "snake_prep", False, False, ("grid_size", "unit_size", "n_foods"), False, ()),
    "Pong": (pong, "pong_prep", True, True, ("points_to_win", "max_episode_steps", "opp_skill_num", "opp_skill_den"), True,
             pong.RULE_KEYS),
    "Breakout": (breakout, "breakout_prep", False, False, ("lives", "max_episode_steps"), True, breakout.RULE_KEYS),
    # the continuous-control world: vector observations, two float actions, Gaussian nets only
    "Point": (point, "null_prep", False, False, ("targets_to_win", "max_episode_steps"), True, point.RULE_KEYS),
    # the pole on a cart: vector observations, two int actions, the discrete FC nets only
    "CartPole": (cartpole, "null_prep", False, False, ("max_episode_steps",), True, cartpole.RULE_KEYS),
    # the pendulum swing-up: vector observations, one float action, Gaussian nets only
    "Pendulum": (pendulum, "null_prep", False, False, ("max_episode_steps",), True, pendulum.RULE_KEYS),
}
# the nets with a Gaussian head (models.py): what a family whose device pool has ``float_actions`` can be trained with
_GAUSS_MODELS = ("FCModel", "GRUFCModel")
# the nets that take a vector observation: with a softmax head, what the CartPole worlds can be trained with
_FC_MODELS = _GAUSS_MODELS
# the families with (1, L) observations: what running normalisation (hyps norm_obs / norm_rewards, section 6m) covers
_VECTOR_WORLDS = ("Point", "CartPole", "Pendulum")
# the keys of section 6i that shape what a policy is TRAINED on, not the game: evaluation worlds do not get them
_TRAINING_ONLY = ("episodic_life", "clip_rewards")


def _float_family(family):
    """does the family's device pool read float action rows (``float_actions``: Point, Pendulum)?"""
    return bool(getattr(getattr(_WORLDS[family][0], "Device" + family + "Pool"), "float_actions", False))


def _world_family(env_type):
    """"Pong" of "Pong-device" / "Pong-host"; None for every other env_type"""
    family, _, where = str(env_type).partition("-")
    return family if family in _WORLDS and where in ("device", "host") else None


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


def train(_, hyps, verbose=True, env_fn=None, eval_env=None, max_epochs=None, uniform_fn=None, on_epoch=None):
    """``hyps``: the reference's flat dict (training_scripts/hyperparams.json; ``n_rollouts`` need not be a multiple of
    ``n_envs``).  ``env_fn(j)`` (optional) builds env j as an object with ``reset()/step(a)`` returning already
    prepped frames -- otherwise gym envs are made from ``env_type`` / ``prep_fxn`` like the reference.  With the
    default process env pool ``env_fn`` travels to the worker processes pickled: lambdas and closures need
    ``cloudpickle`` (else pass a module-level callable, or ``hyps['env_pool'] = 'serial'``).  ``uniform_fn`` /
    ``on_epoch(epoch, updater, shared_data)`` are test hooks (sampler uniforms; called after every update).
    Continuous (``Box``) envs step in this process unless ``hyps['env_pool'] = 'process_f32'``: worker processes behind a
    pool that carries float action vectors (``ProcessEnvPool(action_dim=n)``); ``'process'`` stays the int32 pool.
    ``env_type`` "Snake-device" / "Snake-host" (a2c_amd/snake.py; keys ``grid_size``, ``unit_size``, ``n_foods``) need no
    gym: the first plays ``n_envs`` worlds in device memory (``DeviceSnakePool``), the second ``SnakeEnv``s behind the usual
    ``env_pool`` choices with ``prep_fxn="snake_prep"``; both are evaluated on host ``SnakeEnv``s.
    ``env_type`` "Pong-device" / "Pong-host" (a2c_amd/pong.py; keys ``points_to_win``, ``max_episode_steps``,
    ``opp_skill_num``, ``opp_skill_den``; ``frame_skip``, ``sticky_num``, ``sticky_den``: game frames per step and sticky
    actions, DESIGN.md section 6g, for the Pong and Breakout worlds, training pools and evaluation worlds alike;
    ``frame_skip_max``: the game frames of a step drawn from frame_skip .. frame_skip_max, section 6i, likewise -- with
    ``frame_skip=2, frame_skip_max=4, sticky_num=1, sticky_den=4`` the stepping rule of ``Pong-v0``)
    likewise: ``DevicePongPool``, or ``PongEnv``s behind the usual pools with
    ``prep_fxn="pong_prep"`` (the process pool carries their {0, 1} frames packed, one bit per pixel); 3 actions,
    ``action_shift`` 0 unless given, the "Pong" done override applies, evaluation on host ``PongEnv``s.
    ``env_type`` "Breakout-device" / "Breakout-host" (a2c_amd/breakout.py; keys ``lives``, ``max_episode_steps``, and for the
    training worlds only ``episodic_life``: a lost life closes the step, and ``clip_rewards``: the step's reward is its sign,
    section 6i -- a ValueError on the Pong worlds, as all three keys of that section are on the Snake worlds) likewise:
    ``DeviceBreakoutPool``, or ``BreakoutEnv``s behind the usual pools with ``prep_fxn="breakout_prep"`` (grey levels
    0..255 on the uint8 transport; with ``hyps["device_prep"] = "breakout_prep"`` the process pool carries the RAW frames
    and the device preps them); 4 actions, ``action_shift`` 0 unless given, real dones only, evaluation on host
    ``BreakoutEnv``s.
    ``env_type`` "Point-device" / "Point-host" (a2c_amd/point.py; keys ``targets_to_win``,
    ``max_episode_steps``, ``frame_skip`` / ``frame_skip_max`` / ``sticky_num`` / ``sticky_den`` as on the Pong worlds) are the
    continuous-control world: (1, 8) observations with ``prep_fxn="null_prep"``, ``is_discrete=False``, 2 float actions, for
    ``model`` FCModel / GRUFCModel only (anything else is a ValueError before anything is allocated).  ``DevicePointPool``
    reads the float action rows on the device; "Point-host" steps ``PointEnv``s behind ``env_pool`` "serial" (the default)
    or "process_f32"; evaluation on host ``PointEnv``s.
    ``env_type`` "CartPole-device" / "CartPole-host" (a2c_amd/cartpole.py; keys ``max_episode_steps``,
    ``frame_skip`` / ``frame_skip_max`` / ``sticky_num`` / ``sticky_den`` as on the Pong worlds) are the pole on a cart in this
    project's integer arithmetic ("CartPole-v1" stays gym's): (1, 4) observations with ``prep_fxn="null_prep"``, 2 actions,
    ``action_shift`` 0 unless given, real dones only, for ``model`` FCModel / GRUFCModel with ``is_discrete=True`` only
    (anything else is a ValueError before anything is allocated).  ``DeviceCartPolePool`` reads the sampler's int64 actions
    on the device; "CartPole-host" steps ``CartPoleEnv``s behind the usual pools (the process pool carries their fp32
    frames); evaluation on host ``CartPoleEnv``s.
    ``env_type`` "Pendulum-device" / "Pendulum-host" (a2c_amd/pendulum.py; keys ``max_episode_steps``
    (default 200, at most 2^16), ``frame_skip`` / ``frame_skip_max`` / ``sticky_num`` / ``sticky_den`` as on the Pong worlds) are
    the pendulum swing-up in this project's integer arithmetic ("Pendulum-v1" stays gym's): (1, 4) observations with
    ``prep_fxn="null_prep"``, ``is_discrete=False``, 1 float action (the torque, clamped to +-2), fractional rewards (multiples
    of 2^-8), only the step cap ends an episode, and the same refusals and pools as the Point worlds: ``model`` FCModel /
    GRUFCModel only, "Pendulum-host" behind ``env_pool`` "serial" or "process_f32"; evaluation on host ``PendulumEnv``s.
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
    Returns the best evaluation reward."""
    hyps = dict(DEFAULTS, **hyps)
    # gauss_loss: refused here, before anything is written or allocated, for a value that is neither
    # "reference" nor "exact" and for "exact" where the action space is known to be discrete (a device world's family, an
    # env_fn's is_discrete key; a gym env's space is only known from the probe, where the Updater refuses it)
    world_family = _world_family(hyps.get("env_type")) if env_fn is None else None
    gauss_loss_mode(hyps, (not _float_family(world_family)) if world_family is not None else
                    (bool(try_key(hyps, "is_discrete", True)) if env_fn is not None else None))
    # bootstrap_truncated: refused here, before anything is written or allocated, for everything but the
    # lane worlds' device pools under FCModel
    if try_key(hyps, "bootstrap_truncated", False):
        if env_fn is not None:
            raise ValueError("a2c_amd: bootstrap_truncated bootstraps time-limit episode ends of the lane worlds' device pools, "
                             "not an env_fn's envs")
        check_bootstrap_truncated(hyps)
    eval_pool = try_key(hyps, "eval_pool", None) or "host"
    if eval_pool not in ("host", "device"):
        raise ValueError(f"a2c_amd: hyps['eval_pool'] is 'host' or 'device', not {eval_pool!r}")
    if eval_pool == "device" and (eval_env is not None or env_fn is not None or hyps.get("env_type") not in (
            "Snake-device", "Pong-device", "Breakout-device", "Point-device", "CartPole-device", "Pendulum-device")):
        raise ValueError("a2c_amd: hyps['eval_pool'] = 'device' evaluates the device worlds (env_type 'Snake-device', "
                         "'Pong-device', 'Breakout-device', 'Point-device', 'CartPole-device' or 'Pendulum-device') and takes "
                         "no eval_env / env_fn")
    # running normalisation: the device pools of the vector worlds, evaluated on lock-step twins or on
    # the device; refused here, before anything is written or allocated, for everything else
    norm = vecnorm.norm_settings(hyps)
    if norm is not None:
        key, family = vecnorm.norm_key(hyps), _world_family(hyps.get("env_type"))
        if env_fn is not None or family not in _VECTOR_WORLDS or hyps["env_type"] != family + "-device":
            raise ValueError(f"a2c_amd: {key} normalises inside the rollout slot of a device pool of the vector worlds "
                             f"(env_type {', '.join(repr(f + '-device') for f in _VECTOR_WORLDS)}), not "
                             f"{hyps.get('env_type')!r}" + (" with an env_fn" if env_fn is not None else ""))
        if eval_env is not None:
            raise ValueError(f"a2c_amd: {key} evaluates on lock-step host twins (eval_pool='host') or on the device "
                             "(eval_pool='device'); a single eval_env plays the reference's serial loop, which is not normalised")
    if env_fn is None and _world_family(hyps.get("env_type")) == "Snake":
        if worlds.repeat_from_hyps(hyps, "Snake")[:2] != (1, 0):
            raise ValueError("a2c_amd: frame_skip / sticky_num are keys of the Pong and Breakout worlds: the Snake worlds "
                             "play one game frame per step")
    if env_fn is None and _world_family(hyps.get("env_type")) is not None:
        # frame_skip_max / episodic_life / clip_rewards: refused here, before anything is written or allocated, where the
        # family does not take them or they are out of bounds
        family = _world_family(hyps["env_type"])
        rules = worlds.rules_from_hyps(hyps, family, _WORLDS[family][6])
        if _float_family(family):
            # float actions: the nets with a Gaussian head, never as discrete ones; and no int32 process pool
            n = _WORLDS[family][0].ACTION_SIZE
            if hyps.get("model") not in _GAUSS_MODELS or try_key(hyps, "is_discrete", False):
                raise ValueError(f"a2c_amd: the {family} worlds take {n} float action{'s' if n > 1 else ''}: model "
                                 f"{' / '.join(_GAUSS_MODELS)} with is_discrete=False, not {hyps.get('model')!r}"
                                 + (" with is_discrete=True" if try_key(hyps, "is_discrete", False) else ""))
            if hyps["env_type"] == family + "-host" and try_key(hyps, "env_pool", None) not in (None, "serial", "process_f32"):
                raise ValueError(f"a2c_amd: env_type='{family}-host' steps behind env_pool='serial' (the default) or "
                                 "'process_f32' (the int process pool and the thread pool carry int32 actions)")
        if family == "CartPole":
            # vector observations and two int actions: the FC nets with their softmax head
            if hyps.get("model") not in _FC_MODELS or not try_key(hyps, "is_discrete", True):
                raise ValueError(f"a2c_amd: the CartPole worlds take one of two int actions on (1, 4) observations: model "
                                 f"{' / '.join(_FC_MODELS)} with is_discrete=True, not {hyps.get('model')!r}"
                                 + ("" if try_key(hyps, "is_discrete", True) else " with is_discrete=False"))
    if hyps["n_rollouts"] is None:
        hyps["n_rollouts"] = hyps["n_envs"]
    hyps["main_path"] = try_key(hyps, "main_path", "./")
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

    # environments
    serial = try_key(hyps, "env_pool", "process") == "serial"
    probe = None
    family, raw = _world_family(hyps["env_type"]) if env_fn is None else None, False
    if family is not None:
        mod, prep_name, pong_done, bits, names, repeats, _ = _WORLDS[family]
        world = dict(zip(names, mod.world_from_hyps(hyps)), seed=hyps["seed"])
        if family == "Breakout":
            # device_prep: the workers hand on the RAW frames (null_prep) and a2c_frame_prep_u8 crops / strides them
            raw = try_key(hyps, "device_prep", None) is not None
            if raw and (hyps["device_prep"] != "breakout_prep" or hyps["env_type"] == "Breakout-device" or serial):
                raise ValueError("a2c_amd: device_prep on Breakout worlds is 'breakout_prep', on env_type='Breakout-host' behind "
                                 "the process env pool (the device worlds write prepped frames themselves)")
        hyps["prep_fxn"] = "null_prep" if raw else prep_name
        prep = hyps["preprocessor"] = getattr(preprocessing, hyps["prep_fxn"])
        cont_world = _float_family(family)
        hyps["is_discrete"], n_act = not cont_world, (mod.ACTION_SIZE if cont_world else mod.N_ACTIONS)
        if cont_world:      # a Box: in this process unless env_pool='process_f32' (as below for every continuous env)
            serial = try_key(hyps, "env_pool", None) != "process_f32"
        # a policy that circles never ends its evaluation episode: cap it (StatsRunner reads the key)
        hyps["max_eval_steps"] = try_key(hyps, "max_eval_steps", 2000)
        if repeats:
            world.update(zip(("frame_skip", "sticky_num", "sticky_den"), worlds.repeat_from_hyps(hyps, family)))
        # evaluation plays whole games for the game's score: the dynamics (frame_skip_max), not the training flags
        eval_world = dict(world, **{k: v for k, v in rules.items() if k not in _TRAINING_ONLY})
        world.update(rules)
        factory, device_pool = getattr(mod, family + "Factory"), getattr(mod, "Device" + family + "Pool")
        mk_env = lambda j, kw=world: SequentialEnvironment(hyps["env_type"], getattr(preprocessing, prep_name),
                                                           seed=hyps["seed"], env_fn=factory(env_id=j, **kw))
        side = world["grid_size"] * world["unit_size"] if family == "Snake" else None
        world_shape = (1, side, side) if family == "Snake" else device_pool.frame_shape
        if hyps["env_type"] == family + "-device":
            pool = device_pool(hyps["n_envs"], device=cuda_if(torch.zeros(1)).device, **world)
        elif serial:
            pool = HostEnvPool([mk_env(j) for j in range(hyps["n_envs"])], frame_shape=world_shape)
        else:
            from .hostpool import ProcessEnvPool
            kws = [dict(env_type=hyps["env_type"], preprocessor=prep, seed=hyps["seed"], env_fn=factory(env_id=j, **world))
                   for j in range(hyps["n_envs"])]
            # frame_bits: {0, 1} uint8 planes cross the host link one bit per pixel; grey levels one byte per pixel
            pool = ProcessEnvPool(SequentialEnvironment, hyps["n_envs"], env_kwargs=kws,
                                  n_workers=try_key(hyps, "n_env_workers", None), pong=pong_done,
                                  action_shift=try_key(hyps, "action_shift", 0), frame_bits=bits,
                                  action_dim=n_act if cont_world else None,
                                  # (null_prep puts an axis in front of a twin's (1, L) row: the states are the device pool's)
                                  frame_shape=world_shape if len(world_shape) == 2 else None)
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
    if family is not None:
        pass
    elif env_fn is None:
        kws = [dict({k: v for k, v in hyps.items() if k != "seed"}, seed=hyps["seed"] + j) for j in range(hyps["n_envs"])]
        if serial:
            envs = [SequentialEnvironment(**kw) for kw in kws]
            frame_shape = np.asarray(envs[0].prep_obs(np.zeros(envs[0].raw_shape, dtype=np.uint8))).shape
            pool = HostEnvPool(envs, frame_shape=frame_shape)
        else:
            from .hostpool import ProcessEnvPool
            # pong_prep yields {0,1} uint8 planes (preprocessing.py:15-16): one bit per pixel crosses the host link
            bits = try_key(hyps, "frame_bits", hyps["prep_fxn"] == "pong_prep")
            pool = ProcessEnvPool(SequentialEnvironment, hyps["n_envs"], env_kwargs=kws,
                                  n_workers=try_key(hyps, "n_env_workers", None), pong="Pong" in hyps["env_type"],
                                  action_shift=1 if hyps["env_type"] == "Pong-v0" else try_key(hyps, "action_shift", 0),
                                  frame_bits=bool(bits), action_dim=f32_dim)
    else:
        if serial:
            pool = HostEnvPool([env_fn(j) for j in range(hyps["n_envs"])])
        else:
            from .hostpool import ProcessEnvPool
            pool = ProcessEnvPool(_PositionalFactory(env_fn), hyps["n_envs"], env_kwargs=[dict(j=j) for j in range(hyps["n_envs"])],
                                  n_workers=try_key(hyps, "n_env_workers", None), pong="Pong" in hyps["env_type"],
                                  action_shift=1 if hyps["env_type"] == "Pong-v0" else try_key(hyps, "action_shift", 0),
                                  probe_reset=True, frame_bits=bool(try_key(hyps, "frame_bits", False)), action_dim=f32_dim)
        n_act = hyps["action_size"]
    hyps["state_shape"] = [hyps["n_frame_stack"]] + list(pool.frame_shape[1:])
    if raw:      # the pool carries raw frames: the states are what the device makes of them
        hyps["state_shape"] = [hyps["n_frame_stack"]] + list(world_shape[1:])
    if hyps["env_type"] == "Pong-v0":
        action_size, hyps["action_shift"] = 3, 1                      # training.py:67-69
    else:
        action_size, hyps["action_shift"] = n_act, try_key(hyps, "action_shift", 0)
    hyps["action_size"] = action_size
    shared_len = hyps["n_tsteps"] * hyps["n_rollouts"]
    if verbose:
        print("State Shape:,", hyps["state_shape"], "Num Samples Per Update:", shared_len)

    net = getattr(models, hyps["model"])(hyps["state_shape"], action_size, bnorm=hyps["use_bnorm"],
                                         **{k: v for k, v in hyps.items() if k not in ("use_bnorm",)})
    if hyps["resume"]:
        net.load_state_dict(torch.load(net_save_file))
    net = cuda_if(net)
    net._ensure_device()            # the flat parameter arena exists BEFORE the runner thread and the Updater touch it
    shared_data = {"states": cuda_if(torch.zeros((shared_len, *hyps["state_shape"]))),
                   "deltas": cuda_if(torch.zeros(shared_len)), "rewards": cuda_if(torch.zeros(shared_len)),
                   # (the reference keeps `actions` on the host, training.py:90,97; device resident here so that the
                   # rollout's device relay can write it -- nothing outside this function sees the dict)
                   # (continuous actions: one float row of n per sample, training.py:89-92)
                   "actions": cuda_if(torch.zeros(shared_len).long() if hyps["is_discrete"] else
                                      torch.zeros((shared_len, action_size))),
                   "dones": cuda_if(torch.zeros(shared_len))}
    if net.is_recurrent:
        shared_data["h_states"] = cuda_if(torch.zeros(shared_len, net.h_size))
    if try_key(hyps, "bootstrap_truncated", False):      # (section 6o: indexed like rewards; one observation per row)
        shared_data["truncs"] = cuda_if(torch.zeros(shared_len))
        shared_data["final_obs"] = cuda_if(torch.zeros((shared_len, int(np.prod(pool.frame_shape)))))
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
    # evaluation: the caller's single env (reference loop), else n_test_eps gym envs in lock-step on the device
    if eval_pool == "device":
        # a second pool of the training pool's kind: same world and seed, n_test_eps worlds (DeviceStatsRunner gives them the
        # env ids of the host twins below, and fresh ones on every later call)
        stats_runner = DeviceStatsRunner(hyps, type(pool)(try_key(hyps, "n_test_eps", 15), device=pool.device, **eval_world),
                                         uniform_fn=uniform_fn, norm=eval_norm)
    elif eval_env is not None:
        stats_runner = StatsRunner(hyps, env=eval_env)
    elif family is not None:
        # host twins of worlds the training pool does not play (env ids from 10007 on)
        stats_runner = StatsRunner(hyps, envs=[mk_env(10007 + j, eval_world) for j in range(try_key(hyps, "n_test_eps", 15))],
                                   norm=eval_norm)
    else:
        stats_runner = StatsRunner(hyps) if env_fn is None else None
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
