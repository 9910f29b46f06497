"""Drop-in for the reference's ``a2c/runner.py`` (``SequentialEnvironment``, ``Runner``,
``StatsRunner``), re-designed for one GPU process driving MANY envs in lock-step.

Reference (runner.py:109-248): one OS process per env, batch-1 forwards, every element of the
rollout buffers written one at a time across the host/device boundary.  Here ONE ``Runner``
owns all ``n_envs`` environments: per time step it runs a single batched forward over the B
envs, samples all actions on the device, steps the envs on the host (env stepping stays on the
CPU, frames go up through pinned staging buffers with async copies), and a handful of kernels
write the step's rows of the rollout-major buffers (frame stack -> ``states``, rewards, dones,
TD deltas, ``h_states``).  The ``shared_data`` layout (training.py:88-101) and the gate/stop
queue protocol are unchanged, so ``Updater`` and a ``train()``-style driver see the same data.

Env pools (``env_pool=``):
  * ``hostpool.ProcessEnvPool`` -- the production path: env worker PROCESSES behind one pinned,
    device-mapped region (include/a2c_hostpool.h), frames travel as uint8 when the preprocessor
    yields uint8.  Two ingest modes (``hyps['ingest']`` or ``Runner(..., ingest=)``):
      "zero-copy"  (A3CModel-shaped nets, uint8 frames) the whole slot is ONE persistent launch
                   (a2c_a3c_rollout): workgroups and env workers hand actions / frames to each other
                   through the pinned region, the host process is not in the loop;
      "memcpy"     (every model) per step: actions D2H -> workers step -> hipMemcpyAsync of the
                   frames block from the pinned region into HBM -> the step kernels.
  * ``HostEnvPool`` -- B env objects stepped serially in this process (tests, tiny runs).
  * a *device resident* pool (``device_step`` protocol: frames / rewards / dones already in HBM:
    ``snake.DeviceSnakePool``, or a synthetic tape): a whole n_tsteps rollout is enqueued without a
    single host synchronisation and can be captured into one hipGraph.  ``device_step(t, env0, B)``
    returns (frames (B, HW) fp32, rew, done, reset) device tensors; a pool whose class sets
    ``needs_actions = True`` is called as ``device_step(t, env0, B, actions=(address, stride))`` with
    the int64 actions the sampler just wrote (a pool with ``float_actions``, ``point.DevicePointPool``: the float32 rows of
    ``n_act`` actions a continuous net's a2c_gauss_head wrote, stride in floats), and one with ``episode_stats()`` feeds
    ``rew_q``.  A pool that also has
    ``device_step_post(t, env0, B, actions, post)`` (the Snake / Pong / Breakout worlds: step, bookkeeping and next state
    in one launch) is played as ONE hipGraph per slot when ``hyps['rollout_graphs']`` (default true) and the ``actions``
    buffer is device resident: first rollout eager, second captured, then replayed (``_rollout_block_device``).

``DeviceStatsRunner`` evaluates such a pool on the device (``train()``: ``hyps['eval_pool'] = 'device'``): a private Runner
plays ``n_test_eps`` worlds in chunks, a2c_eval_scan keeps every env's first episode.
"""
import os
import queue
import warnings
import time
from collections import deque

import numpy as np
import torch
import torch.nn.functional as F

from . import families, ops
from .utils import cuda_if, next_state, sample_action, try_key


class SequentialEnvironment:
    """gym adapter with the reference's surface (runner.py:14-106).  ``gym`` is imported lazily;
    ``env_fn`` (optional, not in the reference) lets callers inject any object with
    ``reset()``/``step(a)`` returning raw observations."""

    def __init__(self, env_type, preprocessor, seed=time.time(), float_params=dict(), env_fn=None, **kwargs):
        self.env_type, self.preprocessor, self.seed, self.float_params = env_type, preprocessor, seed, float_params
        if env_fn is not None:
            self.env = env_fn()
        else:
            try:
                import gym
                self.env = gym.make(env_type)
                self.env.seed(self.seed)
            except Exception:
                raise NotImplementedError("Unity compatibility not implemented")
        self.is_gym = True
        self.raw_shape = self.env.reset().shape
        self.is_discrete = hasattr(self.env.action_space, "n")
        self.n = self.env.action_space.n if self.is_discrete else self.env.action_space.shape[0]

    def prep_obs(self, obs):
        return self.preprocessor(obs)

    def reset(self):
        return self.prep_obs(self.env.reset())

    def step(self, action):
        obs, rew, done, info = self.env.step(action)
        return self.prep_obs(obs), rew, done, info

    def render(self):
        return self.env.render()

    def get_action(self, preds, rand_nums=None, noise=None):
        """softmax + inverse-CDF sample of one (or a batch of) logits rows (runner.py:94-97); a continuous env takes the
        ``(mu, sigma)`` tuple and samples mu + sigma*noise (``noise`` default: torch.randn_like(sigma), runner.py:98-104),
        returned as a float32 vector of shape (n,)."""
        if not self.is_gym:
            raise NotImplementedError
        if self.is_discrete:
            probs = F.softmax(preds.detach(), dim=-1)
            return int(sample_action(probs, rand_nums).item())
        mus, sigmas = preds
        if noise is None:
            noise = torch.randn_like(sigmas)
        actions = (mus.detach() + sigmas.detach() * noise.to(sigmas.device)).cpu().squeeze().numpy().astype(np.float32)
        return actions.reshape(1) if actions.ndim == 0 else actions


class HostEnvPool:
    """B host environments stepped one after the other on the CPU (the reference's env stepping,
    runner.py:208, stays on the host).  Observations are the already prepped (1,H,W) frames."""

    def __init__(self, envs, frame_shape=None):
        self.envs = list(envs)
        if frame_shape is None:
            # raw envs: one probing reset each, exactly what SequentialEnvironment.__init__ does
            # to read raw_shape (runner.py:45)
            frame_shape = np.asarray(self.envs[0].reset()).shape
            for e in self.envs[1:]:
                e.reset()
        self.frame_shape = tuple(frame_shape)

    def __len__(self):
        return len(self.envs)

    def reset(self, j):
        return np.asarray(self.envs[j].reset())

    def step(self, j, action):
        obs, rew, done, _ = self.envs[j].step(action)
        return np.asarray(obs), float(rew), bool(done)


def gym_env_pool(hyps, n_envs, seed, serial, action_shift, rew_ema0, action_dim=None):
    """``n_envs`` gym envs made from the hyps like the reference's n_envs processes (training.py:109-121), env j seeded
    ``seed + j``: in this process (``serial``), else worker processes behind the pinned pool region -- with ``action_dim``
    the pool of float action vectors.  The one builder of ``Runner._make_pool`` and ``train()``"""
    kws = [dict({k: v for k, v in hyps.items() if k != "seed"}, seed=seed + j) for j in range(n_envs)]
    if serial:
        envs = [SequentialEnvironment(**kw) for kw in kws]
        return HostEnvPool(envs, frame_shape=np.asarray(envs[0].prep_obs(np.zeros(envs[0].raw_shape, dtype=np.uint8))).shape)
    from .hostpool import ProcessEnvPool
    # pong_prep yields {0,1} uint8 planes (preprocessing.py:15-16): one bit per pixel crosses the host link
    bits = try_key(hyps, "frame_bits", try_key(hyps, "prep_fxn", None) == "pong_prep")
    return ProcessEnvPool(SequentialEnvironment, n_envs, env_kwargs=kws, n_workers=try_key(hyps, "n_env_workers", None),
                          action_shift=action_shift, pong="Pong" in hyps["env_type"], rew_ema0=rew_ema0, frame_bits=bool(bits),
                          action_dim=action_dim)


class _Frames:
    """Where the new frames of one env step are on the device: fp32 (B, HW) or uint8 (B, stride bytes)."""
    __slots__ = ("ptr32", "ptr8", "stride")

    def __init__(self, ptr32=0, ptr8=0, stride=0):
        self.ptr32, self.ptr8, self.stride = ptr32, ptr8, stride


def env_action(na_j, shift, cont):
    """what env.step receives: int(action) + shift, or the float32 (n,) vector + shift"""
    if cont:
        return na_j + np.float32(shift)
    return int(na_j) + shift


def host_env_step(pool, env0, B, np_act, np_frames, np_rew, np_done, ep_rew, rew_q, shift, pong, cont):
    """Envs env0..env0+B of an in-process pool take one step (runner.py:208-232): actions from rows env0.. of the numpy view
    ``np_act`` (``env_action``: int, or with ``cont`` float rows), frames / rewards / dones into the same rows of the other
    views.  ``ep_rew`` sums each env's rewards; an episode's end folds the sum into the EMA that ``rew_q`` holds.  With
    ``pong`` a non-zero reward ends the agent's episode, not the env's: no reset, done row 0."""
    for j in range(env0, env0 + B):
        obs, rew, done = pool.step(j, env_action(np_act[j], shift, cont))
        ep_rew[j] += rew
        reset = done
        if pong and rew != 0:
            done = True
        if done and rew_q is not None:                                 # runner.py:216-217
            rew_q.put(.99 * rew_q.get() + .01 * ep_rew[j])
        if done:
            ep_rew[j] = 0
        if reset:
            obs = pool.reset(j)
        np_frames[j] = np.asarray(obs, dtype=np.float32).reshape(-1)
        np_rew[j], np_done[j] = rew, float(reset)


def check_bootstrap_truncated(hyps, pool=None, net=None, datas=None, HW=None):
    """what hyps['bootstrap_truncated'] = True refuses, each with a ValueError naming the key; every
    argument is optional, so train() asks before anything is allocated and the Runner again with what it was handed.  The
    lane worlds' device pools (``reports_trunc``) and FCModel only: a recurrent net would need the hidden row the post step
    zeroes, a picture world a second rendered frame per close, and the host pools carry no such field"""
    key = "bootstrap_truncated"
    env_type = hyps.get("env_type")
    if pool is None:
        if env_type not in families.LANE_DEVICE_TYPES:
            raise ValueError(f"a2c_amd: {key} bootstraps time-limit episode ends of the lane worlds' device pools (env_type "
                             f"{', '.join(map(repr, families.LANE_DEVICE_TYPES))}), not {env_type!r}")
    elif not getattr(pool, "reports_trunc", False):
        raise ValueError(f"a2c_amd: {key} needs a device env pool whose step reports the state an episode ended in "
                         f"({', '.join(families.FAMILIES[n].pool.__name__ for n in families.LANE_WORLDS)}), not "
                         f"{type(pool).__name__}")
    model = type(net).__name__ if net is not None else hyps.get("model")
    if model is not None and model != "FCModel":
        raise ValueError(f"a2c_amd: {key} covers FCModel (the hidden row a recurrent net's final state needs is zeroed before "
                         f"anyone can read it), not {model}")
    if datas is not None:
        n = datas["rewards"].numel()
        for name, shape in (("truncs", (n,)), ("final_obs", (n, HW))):
            t = datas.get(name)
            if t is None or tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_cuda:
                raise ValueError(f"a2c_amd: {key} needs shared_data[{name!r}], a float32 device tensor of shape {shape}")


def play_graph(cache, key, body):
    """The one graph state machine of the rollout paths.  ``body()`` only enqueues.  First call of ``key``: ``body()`` runs
    eagerly (the conv tile tuners measure on eager calls) and the key is "warm"; second call: captured into a
    torch.cuda.CUDAGraph, stored and replayed; later calls: replayed.  A capture that raises stores False, for good.
    -> what ``cache[key]`` now holds; on False nothing was played and the caller decides what is."""
    g = cache.get(key)
    if g is None:
        cache[key] = "warm"
        body()
        return "warm"
    if g == "warm":
        try:
            g = torch.cuda.CUDAGraph()
            with ops.graph_capture(g):
                body()
            cache[key] = g
        except Exception:      # noqa: BLE001 -- capture not possible here
            torch.cuda.synchronize()
            g = cache[key] = False
    if g:
        g.replay()
    return g


class _Slot:
    """One block of a rollout: slots slot0..slot0+B played by envs env0..env0+B for T steps -- what every rollout path
    reads, built once in ``Runner._rollout_block``.  The segmented path adds its own fields (``_rollout_block_segmented``)."""

    def __init__(self, r, net, slot0, env0, B, hyps):
        D = r.datas
        self.r, self.net, self.slot0, self.env0, self.B, self.hyps = r, net, slot0, env0, B, hyps
        self.T, self.S = int(hyps["n_tsteps"]), r.S
        self.gamma, self.pong, self.shift = hyps["gamma"], "Pong" in hyps["env_type"], hyps["action_shift"]
        self.bm = r.bookmark[env0:env0 + B]
        self.val_prev, self.done_eff = r.val_prev[env0:env0 + B], r.done_eff[env0:env0 + B]
        self.h = None if r.h is None else r.h[env0:env0 + B]
        self.act = r.act_dev[env0:env0 + B]
        self.acts_host_out = D["actions"] if not D["actions"].is_cuda else None
        # recurrent nets: bookkeeping + frame stack + hidden-state reset + the h_states row in ONE launch (a2c_rollout_post_rec,
        # .._post_frames); GRUModel's cell stash needs it
        self.fused_post = (self.h is not None and r.HW % 4 == 0 and r.S % 4 == 0
                           and os.environ.get("A2C_NO_FUSED_POST") != "1")
        self.fused = self.relay = self.lazy = False
        self.stash = self.ub = self.fs = self.post_done = None

    def sp(self, t):
        """address of states[slot0*T + t]; the B slots' rows are T*S floats apart"""
        return self.r.datas["states"].data_ptr() + 4 * (self.slot0 * self.T + t) * self.S

    def nxt(self, t):
        """(address, row stride) of the state after env step t: states[slot0*T + t + 1], or the bookmark after the last"""
        return (self.sp(t + 1), self.T * self.S) if t + 1 < self.T else (self.bm.data_ptr(), self.S)

    def act_row(self, t):
        """(address, element stride) of datas['actions'][slot0*T + t] for B slots T rows apart (int64 or float rows of n)"""
        a, n = self.r.datas["actions"], self.r.n_act
        if self.r.cont:
            return a.data_ptr() + 4 * n * (self.slot0 * self.T + t), self.T * n
        return a.data_ptr() + 8 * (self.slot0 * self.T + t), self.T

    def act_dst(self, t):
        """where the sampler writes the actions of step t: in place into a device-resident actions buffer, else staging"""
        if self.acts_host_out is None:
            return self.act_row(t)
        return self.act.data_ptr(), (self.r.n_act if self.r.cont else 1)

    def h_row(self, t):
        """(address, row stride) of datas['h_states'][slot0*T + t] (recurrent nets)"""
        hd = self.h.shape[1]
        return self.r.datas["h_states"].data_ptr() + 4 * (self.slot0 * self.T + t) * hd, self.T * hd

    def trunc(self, t):
        """the ``ops.world_trunc`` block of env step t under hyps bootstrap_truncated: row
        slot0 * T + t of datas['truncs'] / datas['final_obs'], the B slots' rows T and T * HW floats apart; else None"""
        if not self.r.trunc:
            return None
        D, HW, e = self.r.datas, self.r.HW, self.slot0 * self.T + t
        return ops.world_trunc(D["truncs"].data_ptr() + 4 * e, self.T, D["final_obs"].data_ptr() + 4 * e * HW, self.T * HW)

    def acts_to_host_out(self, t, src):
        """a host `actions` tensor like the reference's: step t's rows of the B slots"""
        if self.acts_host_out is not None:
            self.acts_host_out[self.slot0 * self.T + t:(self.slot0 + self.B) * self.T:self.T] = src


class Runner:
    """Collects rollouts for ALL envs of this process into ``datas`` (reference signature:
    runner.py:110).  ``datas`` tensors should live on the device (``cuda_if`` them like
    training.py:94-101); ``actions`` may stay a host LongTensor like the reference's."""

    def __init__(self, datas, hyps, gate_q, stop_q, rew_q, env_pool=None, uniform_fn=None, ingest=None, normal_fn=None,
                 stash=True, bootstrap=True, frozen_norm=None, ranks=None):
        self.hyps, self.datas = hyps, datas
        # running normalisation (hyps norm_obs / norm_rewards): the DeviceVecNorm block this Runner owns
        # and advances behind every step's post launch, made in start().  frozen_norm: an evaluation's Runner
        # (DeviceStatsRunner) normalises its observations by the TRAINING Runner's block instead, and writes nothing to it
        self.vecnorm, self._norm, self._norm_frozen = frozen_norm, None, frozen_norm is not None
        self.norm_state = None                # a RunningNorm / its state_dict to start the block from (train(): resume)
        # ranks: ``Shard.world`` of a sharded run (normalisation is refused above one rank: the ranks' moments would drift
        # apart); None: the initialised process group's size, 1 without one
        self.ranks = ranks
        # an evaluation's Runner (DeviceStatsRunner) plays a net between a training rollout and its update: stash=False leaves
        # what that rollout stashed in the net for the update alone; bootstrap=False leaves the last step's rewards / dones
        # rows as the env returned them (no runner.py:236-245) -- device pools with ``device_step_post`` only
        self.stash, self.bootstrap = bool(stash), bool(bootstrap)
        self.trunc = False                    # hyps bootstrap_truncated, once start() has checked it
        self.gate_q, self.stop_q, self.rew_q = gate_q, stop_q, rew_q
        self.obs_deque = deque(maxlen=hyps["n_frame_stack"])     # kept for API parity (single-env helpers)
        self.env_pool = env_pool
        self.uniform_fn = uniform_fn          # (t, B) -> device tensor (B,) of uniforms; default torch.rand
        self.normal_fn = normal_fn            # continuous nets: (t, B, env0) -> device tensor (B, n) of N(0,1); default torch.randn
        self.ingest = ingest or try_key(hyps, "ingest", None)     # None: zero-copy when it applies, else memcpy
        self._ready = False
        self.error = None                     # exception that ended run() (training.train re-raises it)
        self.proc_pool = self.device_pool = False     # (what the env pool is: start())
        self.dev_prep = None
        self._warned_partial = False
        # what the rollout paths keep between calls: the slot's persistent noise (T, n_envs) / (T, n_envs, n), the relay's
        # step counter, action staging, the frame store, and the graphs of the device (whole slot) and host (segment) paths:
        # key -> "warm" (played eagerly once), a torch.cuda.CUDAGraph, or False (capture failed: eager for good)
        self._u_buf = self._e_buf = self._seq_dev = self._act_gather = self._acts_dev = self._fstore = None
        self._fstore_ok = True
        self._states_stale = self._lm_written = False
        self._frames_written = None
        self._dev_graphs, self._seg_graphs = {}, {}

    # ------------------------------------------------------------------ set-up (body of run())
    def _make_pool(self):
        """n_envs gym envs like the reference's n_envs processes (training.py:109-121): worker processes
        behind the pinned pool region; ``hyps['env_pool'] == 'serial'`` keeps them in this process."""
        hyps = self.hyps
        return gym_env_pool(hyps, int(try_key(hyps, "n_envs", 1)), try_key(hyps, "seed", 0),
                            try_key(hyps, "env_pool", "process") == "serial", action_shift=hyps["action_shift"], rew_ema0=-1.0)

    def start(self, net):
        """Everything Runner.run does before its loop (runner.py:158-168), for all envs."""
        self.net = net
        net._ensure_device()
        dev = net._dev
        hyps = self.hyps
        if self.env_pool is None:
            self.env_pool = self._make_pool()
        pool = self.env_pool
        B = self.B = len(pool)
        C = int(hyps["n_frame_stack"])
        fshape = tuple(pool.frame_shape)          # (1, H, W) or (1, L)
        # hyps['device_prep'] = "pong_prep" / "breakout_prep" (SURVEY.md 8 row f4): the envs hand on RAW (H, W, C) uint8
        # frames (host preprocessor = null_prep) and a2c_frame_prep_u8 crops / strides / binarises them on the device
        self.dev_prep = try_key(hyps, "device_prep", None)
        if self.dev_prep:
            if self.dev_prep not in ops.PREP_SPECS or len(fshape) < 3:
                raise ValueError("device_prep: 'pong_prep' or 'breakout_prep' on raw (H, W, C) frames")
            self.raw_dims = tuple(int(v) for v in fshape[-3:])
            fshape = ops.prep_out_shape(self.dev_prep, self.raw_dims[0], self.raw_dims[1])
        self.C, self.HW = C, int(np.prod(fshape))
        self.state_shape = (C,) + fshape[1:]
        self.S = C * self.HW
        self.device_pool = hasattr(pool, "device_step")
        self.proc_pool = hasattr(pool, "post_actions")
        if not self.bootstrap and not hasattr(pool, "device_step_post"):
            raise ValueError("a2c_amd.Runner: bootstrap=False needs a device env pool with device_step_post")
        from . import vecnorm as vn
        if self._norm_frozen:
            self._norm = dict(obs=True, rewards=False)
        else:
            vn.check_runner(hyps, pool, net, getattr(net, "_step_supported", lambda: False)(), ranks=self.ranks)
            self._norm = vn.norm_settings(hyps)
            if self._norm is not None:
                self.vecnorm = vn.DeviceVecNorm(fshape[1], B, hyps["gamma"], eps=self._norm["eps"],
                                                clip_obs=self._norm["clip_obs"], clip_rew=self._norm["clip_rew"], device=dev)
                if self.norm_state is not None:
                    self.vecnorm.load(self.norm_state)
        # continuous nets (is_discrete=False): actions are float rows of n, sampled by a2c_gauss_head
        self.cont = not getattr(net, "is_discrete", True)
        self.n_act = int(net.output_space)
        # ... over a process pool they travel as float action granules (ProcessEnvPool(action_dim=n), a2c_hostpool.h)
        if self.cont and self.proc_pool and int(getattr(pool, "act_dim", 0) or 0) != self.n_act:
            raise ValueError("a2c_amd.Runner: a continuous-action net needs an in-process (HostEnvPool) or device env pool, or "
                             "a ProcessEnvPool(action_dim=n) with n = the net's action size; the int process pool and the "
                             "thread env pool carry int32 actions")
        if not self.cont and int(getattr(pool, "act_dim", 0) or 0):
            raise ValueError("a2c_amd.Runner: a pool with float action granules (action_dim) needs a continuous-action net")
        # ... and a device pool with ``float_actions`` (point.DevicePointPool) reads the float rows where the sampler wrote them
        self.float_pool = bool(getattr(pool, "float_actions", False))
        if self.cont and getattr(pool, "needs_actions", False) and not self.float_pool:
            raise ValueError("a2c_amd.Runner: an action-driven device env pool reads int64 actions; the net is continuous")
        if self.float_pool and not self.cont:
            raise ValueError("a2c_amd.Runner: a device env pool with float actions needs a continuous-action net "
                             "(is_discrete=False)")
        if self.float_pool and int(pool.n_act) != self.n_act:
            raise ValueError(f"a2c_amd.Runner: the device env pool takes {int(pool.n_act)} float actions, the net has "
                             f"{self.n_act}")
        # time-limit truncation (hyps bootstrap_truncated): the lane worlds' step also writes row t of
        # datas['truncs'] / datas['final_obs'] for the update.  An evaluation's Runner (bootstrap=False) never asks
        self.trunc = bool(try_key(hyps, "bootstrap_truncated", False)) and self.bootstrap
        if self.trunc:
            check_bootstrap_truncated(hyps, pool=pool, net=net, datas=self.datas, HW=self.HW)
        f32 = dict(dtype=torch.float32, device=dev)
        self.bookmark = torch.zeros((B, self.S), **f32)                  # state_bookmark of every env
        self.val_prev = torch.zeros(B, **f32)
        self.done_eff = torch.zeros(B, **f32)
        self.act_dev = torch.zeros((B, self.n_act), **f32) if self.cont else torch.zeros(B, dtype=torch.int64, device=dev)
        self.h = torch.zeros((B, net.h_size), **f32) if net.is_recurrent else None   # h_bookmark
        self.ep_rew = np.zeros(B)
        pin = torch.cuda.is_available()
        mk = lambda *s, dt=torch.float32: (torch.zeros(*s, dtype=dt).pin_memory() if pin else torch.zeros(*s, dtype=dt))
        ones = torch.ones(B, **f32)
        if self.proc_pool:
            # worker processes behind the pinned region: frame 0 of every env (its env.reset()) is already there
            pool.start()
            self.h_rew, self.h_done = mk(B), mk(B)
            self.h_act = mk(B, self.n_act) if self.cont else mk(B, dt=torch.int64)
            self.np_rew, self.np_done, self.np_act = self.h_rew.numpy(), self.h_done.numpy(), self.h_act.numpy()
            self.d_rew, self.d_done = torch.zeros(B, **f32), torch.zeros(B, **f32)
            self.u8 = pool.frame_dtype == np.uint8
            self.bits = bool(getattr(pool, "frame_bits", False))      # packed transport: one bit per pixel over the link
            self.fstride = int(pool.header.frame_stride)              # bytes between the envs' slots in the pinned region
            if self.bits and self.HW % 16:
                raise ValueError("frame_bits transport: the frame size must be a multiple of 16 pixels")
            if self.dev_prep and (not self.u8 or self.bits or self.fstride % 16):
                raise ValueError("device_prep needs a uint8 (not packed) raw-frame pool")
            # HBM staging of one env step's frames: uint8 pixels (expanded from the packed slots on the way in), or fp32
            self.dstride = -(-self.HW // 16) * 16 if (self.bits or self.dev_prep) else self.fstride
            self.d_frames = torch.zeros((B, self.dstride), dtype=torch.uint8, device=dev)
            self.d_raw = torch.zeros((B, self.fstride), dtype=torch.uint8, device=dev) if self.dev_prep else None
            self.d_packed = torch.zeros((B, self.fstride), dtype=torch.uint8, device=dev) if self.bits else None
            # fp32 frames whose size is not a multiple of 16 B sit `fstride` bytes apart; the fp32 frame-stack kernels
            # read dense (B, HW) rows: compact them with one strided row copy
            self.d_dense = torch.zeros((B, self.HW), **f32) if (not self.u8 and self.fstride != 4 * self.HW) else None
            self.rollout_err = torch.zeros(1, dtype=torch.int32, device=dev)
            pool.set_phase(1)
            pool.wait_frames(pool.seq_start)
            fr = self._pool_frames_h2d(pool, 0, B, ops.stream())
            if fr.ptr8:
                ops.frame_stack_push_u8(fr.ptr8, fr.stride, ones, self.bookmark.data_ptr(), self.S, self.bookmark.data_ptr(),
                                        self.S, B, C, self.HW)
            else:
                ops.frame_stack_push(_Ptr(fr.ptr32), ones, self.bookmark.data_ptr(), self.S, self.bookmark.data_ptr(), self.S,
                                     B, C, self.HW)
            torch.cuda.current_stream().synchronize()
        elif not self.device_pool:
            self.h_frames, self.h_rew, self.h_done, self.h_reset = mk(B, self.HW), mk(B), mk(B), mk(B)
            self.h_act = mk(B, self.n_act) if self.cont else mk(B, dt=torch.int64)
            self.np_frames, self.np_rew, self.np_done, self.np_act = (x.numpy() for x in (self.h_frames, self.h_rew,
                                                                                             self.h_done, self.h_act))
            self.d_frames = torch.zeros((B, self.HW), **f32)
            self.d_rew, self.d_done, self.d_reset = (torch.zeros(B, **f32) for _ in range(3))
            # initial state: next_state(reset=True) -> [0,..,0, env.reset()] (utils.py:37-42)
            for j in range(B):
                self.np_frames[j] = np.asarray(pool.reset(j), dtype=np.float32).reshape(-1)
            self.d_frames.copy_(self.h_frames, non_blocking=True)
            ops.frame_stack_push(self.d_frames, ones, self.bookmark.data_ptr(), self.S, self.bookmark.data_ptr(), self.S,
                                 B, C, self.HW)
        else:
            pool.start(self)
            if self._norm is not None and self._norm["obs"]:      # the first observation, behind its frame_stack_push
                self.vecnorm.launch(B, 0, out_ptr=self.bookmark.data_ptr(), out_stride=self.S, C=C,
                                    update=not self._norm_frozen)
        for p in net.parameters():
            p.requires_grad = False
        self._ready = True

    def run(self, net):
        """Entry point with the reference's protocol: wait on gate_q, roll out, answer on stop_q.
        An exception ends the loop, is kept in ``self.error`` and is answered with ``None`` tokens on
        stop_q so that the consumer wakes up (the reference's dead runner process deadlocks its
        ``stop_q.get()`` forever)."""
        try:
            self.start(net)
            while True:
                idxs = [self.gate_q.get()]
                if idxs[0] is None:        # shutdown token
                    return
                # the driver re-opens the gate with ALL n_rollouts tokens in one go (training.py:122-123, 174-175): take
                # the whole epoch, so that the slot -> env assignment below is the same every epoch.  Fewer tokens
                # (a caller that trickles them) still work: whatever arrived is played in lock-step rounds.
                n_tok = int(try_key(self.hyps, "n_rollouts", None) or self.B)
                stop = False
                # The rest of the epoch's tokens: wait for them (a partial batch would be played with a different
                # slot -> env mapping, which defeats the activation stash and captures a second set of slot graphs) --
                # but never forever: after hyps["gate_timeout_s"] without a further token (default 5 s; 0.05 s when the
                # caller did not say how many slots an epoch has, i.e. no "n_rollouts" key) whatever arrived is played,
                # so a caller that trickles fewer tokens, or two Runners sharing one gate_q, make progress and their
                # stop_q consumers wake up.
                gate_to = try_key(self.hyps, "gate_timeout_s", None)
                if gate_to is None:
                    gate_to = 5.0 if try_key(self.hyps, "n_rollouts", None) else 0.05
                while len(idxs) < n_tok:
                    try:
                        tok = self.gate_q.get(timeout=gate_to)
                    except queue.Empty:
                        # ONE Runner per gate_q is what performs: Runners sharing a gate_q (the reference's topology) each
                        # take part of the epoch's tokens, stall here once per epoch and play partial batches (which also
                        # re-capture slot graphs and defeat the activation stash).  Say so instead of stalling silently.
                        if not self._warned_partial:
                            self._warned_partial = True
                            warnings.warn("a2c_amd.Runner: %d of %d gate tokens after %.2f s -- playing a partial batch; use ONE "
                                          "Runner per gate_q (or set hyps['gate_timeout_s'])" % (len(idxs), n_tok, gate_to),
                                          RuntimeWarning)
                        break
                    if tok is None:
                        stop = True
                        break
                    idxs.append(tok)
                self.rollout(net, sorted(idxs), self.hyps)
                self.finish()
                for i in idxs:
                    self.stop_q.put(i)
                if stop:
                    return
        except BaseException as e:      # noqa: BLE001
            self.error = e
            for _ in range(int(try_key(self.hyps, "n_rollouts", 1))):
                try:
                    self.stop_q.put_nowait(None)
                except Exception:      # noqa: BLE001
                    break
            raise

    def finish(self):
        """Wait for the enqueued rollout work, surface a host-handshake timeout of the persistent kernel,
        publish the episode-reward EMA the env workers kept (runner.py:216) and let the workers idle."""
        torch.cuda.current_stream().synchronize()
        if self.proc_pool:
            if not (self.env_pool.dev_phase and self.datas["actions"].is_cuda):
                self.env_pool.set_phase(0)
            self.check()
            if self.rew_q is not None:
                self.rew_q.get()
                self.rew_q.put(self.env_pool.rew_ema())
        elif self.device_pool and self.rew_q is not None and hasattr(self.env_pool, "episode_stats"):
            # the pool counted finished episodes and summed their rewards on the device: ONE read per rollout.  The k
            # episodes enter the EMA of runner.py:216 together, as k updates with their mean
            k, total = self.env_pool.episode_stats()
            if k:
                self.rew_q.put(.99 ** k * self.rew_q.get() + (1 - .99 ** k) * total / k)

    def check(self):
        if self.proc_pool and int(self.rollout_err.item()):
            self.env_pool._check_workers()
            raise TimeoutError("a2c_a3c_rollout: an env worker did not answer within the time-out")

    def close(self):
        if self.proc_pool:
            self.env_pool.close()

    # ------------------------------------------------------------------ the rollout
    def rollout(self, net, idx, hyps):
        """Fill slot(s) ``idx``: an int like the reference (runner.py:174), or a list of slots of ANY length.  The
        list is played in lock-step ROUNDS of at most n_envs slots: slot k of a round is played by env k (the
        reference hands slots to whichever of its n_envs runner processes is free, runner.py:169-172; n_rollouts
        need not be a multiple of n_envs -- its shipped hyperparams.json has 45 / 11).  Inside a round, runs of
        contiguous slots whose envs have taken the same number of steps go through ONE batched block."""
        if not self._ready:
            self.start(net)
        idxs = [idx] if isinstance(idx, int) else list(idx)
        N = self.datas["states"].shape[0]
        T_ = int(hyps["n_tsteps"])
        # rows a lazy rollout (hyps['lazy_states']) left in the single-frame store only: a partial refill keeps the others
        if self._states_stale:
            if idxs == list(range(N // T_)):
                self._states_stale = False
            else:
                self.materialize_states()
        # whatever an earlier rollout stashed in the net describes states this call overwrites
        if self.stash:
            net._stash = None
            net._stash_frames = None
            net._stash_lm = False
            if hasattr(net, "_cells_done"):
                net._cells_done = -1
        self._lm_written = False
        # a call that fills EVERY row of the rollout buffer: the step kernels may stash the conv activations
        # of each state for the update that follows (same weights, same states)
        self._stash_bufs = None
        self._frames_written = None
        if self.stash and idxs == list(range(N // T_)) and N % T_ == 0:
            self._stash_bufs = net.stash_rows(self.datas["states"], N, T=T_)
        stash_all = self._stash_bufs is not None
        seqs = self.env_pool.seq_env if self.proc_pool else None
        # the env workers spin on their cmd granules only while a rollout is running: the phase word of the pool is
        # written FROM THE STREAM (in order with the rollout kernels -- the host may be enqueueing this rollout while the
        # previous update still runs), by the host when the region is not device mapped
        dev_phase = self.env_pool.dev_phase if (self.proc_pool and self.datas["actions"].is_cuda) else 0
        if dev_phase:
            ops.store_u32_system(dev_phase, 1)
        elif self.proc_pool:
            self.env_pool.set_phase(1)
        try:
            for r0 in range(0, len(idxs), self.B):
                rnd = idxs[r0:r0 + self.B]
                j = 0
                while j < len(rnd):
                    k = j
                    while k + 1 < len(rnd) and rnd[k + 1] == rnd[k] + 1 and (seqs is None or seqs[k + 1] == seqs[j]):
                        k += 1
                    self._rollout_block(net, rnd[j], j, k - j + 1, hyps)
                    stash_all = stash_all and self._stash_used
                    if self.proc_pool:
                        self.env_pool.advance(j, k - j + 1, T_)
                    j = k + 1
        except BaseException:
            # an env time-out, a lock-step violation or a failed capture must not leave the workers spinning on their cmd
            # granules until close(): back to the sleeping phase from the HOST (the stream may be unusable)
            if self.proc_pool:
                try:
                    self.env_pool.set_phase(0)
                except Exception:      # noqa: BLE001
                    pass
            raise
        if dev_phase:       # ... the last env step has been played: the workers sleep-poll through the update
            ops.store_u32_system(dev_phase, 0)
        if stash_all:
            if self._lm_written:      # (A3CModel, ring kernel: lane masks of a1 beside the stash)
                net.stash_commit(self.datas["states"], N, frames=self._frames_written, lanemask=True)
            else:
                net.stash_commit(self.datas["states"], N, frames=self._frames_written)

    def _uniforms(self, t, B, env0):
        if self.uniform_fn is not None:
            return self.uniform_fn(t, B, env0)
        return torch.rand(B, device=self.net._dev, dtype=torch.float32)

    def _normals(self, t, B, env0):
        if self.normal_fn is not None:
            return self.normal_fn(t, B, env0).reshape(B, self.n_act)
        return torch.randn((B, self.n_act), device=self.net._dev, dtype=torch.float32)

    def _slot_noise(self, T, env0, B):
        """the slot's noise in ONE persistent buffer each (rows are what graph nodes read), filled before the slot and outside
        any graph: uniforms ``_u_buf`` (T, n_envs); continuous nets: N(0,1) ``_e_buf`` (T, n_envs, n) instead"""
        dev = self.net._dev
        if self._u_buf is None or self._u_buf.shape != (T, self.B):
            self._u_buf = torch.zeros((T, self.B), dtype=torch.float32, device=dev)
        ub = self._u_buf
        if self.cont:
            n = self.n_act
            if self._e_buf is None or self._e_buf.shape != (T, self.B, n):
                self._e_buf = torch.zeros((T, self.B, n), dtype=torch.float32, device=dev)
            for t in range(T):
                self._e_buf[t, env0:env0 + B].copy_(self._normals(t, B, env0))
        elif self.uniform_fn is not None:
            for t in range(T):
                ub[t, env0:env0 + B].copy_(self.uniform_fn(t, B, env0).reshape(B))
        else:
            ub[:, env0:env0 + B] = torch.rand((T, B), device=dev, dtype=torch.float32)
        return ub

    def _sample(self, net, logits, u, eps, a_ptr, a_stride, B, st, pub=None):
        """actions of the step from the policy heads: softmax sampling, or mu + sigma*eps (a2c_gauss_head).  pub = (act, act_stride,
        cmd, seq_base, seq_off), continuous nets behind the device relay: the sampling threads hand the actions to the env
        workers themselves (a2c_gauss_head_publish) -- no publish launch behind this one"""
        if self.cont and pub is not None:
            ops.gauss_head_publish(logits, self.n_act, B, eps, a_ptr, a_stride, *pub, st=st)
        elif self.cont:
            ops.gauss_head(logits, self.n_act, B, eps=eps, actions_ptr=a_ptr, act_ld=a_stride, st=st)
        else:
            ops.softmax_sample(logits, u, a_ptr, a_stride, B, net.output_space, st=st)

    def _forward(self, net, x_ptr, bstride, B, env0, st, sampler=None, stash=None):
        """stash = (bufs, row0, row_stride): conv-stack nets write this step's activations into the update's buffers"""
        kw = dict(stash=stash) if (stash is not None and isinstance(stash[0], list)) else {}
        if sampler is not None and getattr(net, "_fused_sampling", False):
            kw["sampler"] = sampler
        if net.is_recurrent:
            return net._fwd(x_ptr, bstride, B, "roll", st, False, h_in=self.h[env0:env0 + B], **kw)
        return net._fwd(x_ptr, bstride, B, "roll", st, False, **kw)

    def _zero_copy_ok(self, net):
        """the persistent one-launch rollout applies: A3CModel-shaped net, process pool with uint8 frames"""
        if not self.proc_pool or self.h is not None or self.ingest in ("memcpy", "relay") or self.dev_prep:
            return False
        ok = (getattr(net, "_step_supported", lambda: False)() and self.u8 and self.HW % 16 == 0 and self.HW <= 8192
              and self.env_pool.dev_ptr != 0)
        if self.ingest == "zero-copy" and not ok:
            raise ValueError("ingest='zero-copy' needs an A3CModel-shaped net (a2c_a3c_step_supported) and a registered "
                             "process env pool with uint8 frames")
        return ok

    def _policy_step(self, c, t, a_ptr, a_stride, st, noise=None):
        """one env step of the policy on state t of the slot: the h_states row (recurrent nets, runner.py:201), the forward
        with its sampler, the sampling launch unless the forward sampled, the new hidden rows back into ``h`` unless the net
        updated them in place.  noise = (u, eps) rows of the slot's persistent buffers; None: drawn here, per step.
        -> the forward's outputs"""
        net, h, B, env0 = c.net, c.h, c.B, c.env0
        if h is not None:
            hd = h.shape[1]
            ops.copy_rows(h.data_ptr(), hd, *c.h_row(t), B, hd, st)
        if noise is None:
            noise = (None, self._normals(t, B, env0)) if self.cont else (self._uniforms(t, B, env0), None)
        u, eps = noise
        out = self._forward(net, c.sp(t), c.T * c.S, B, env0, st, sampler=None if self.cont else (u, a_ptr, a_stride))
        if not out.get("sampled", False):
            self._sample(net, out["logits"], u, eps, a_ptr, a_stride, B, st)
        if h is not None and out["h"].data_ptr() != h.data_ptr():      # (the GRU models update h in place)
            ops.copy_rows(out["h"].data_ptr(), h.shape[1], h.data_ptr(), h.shape[1], B, h.shape[1], st)
        return out

    def _step_args(self, c, k, fr, rew, done, reset, stash):
        """keyword block of ``net._step`` (a2c_a3c_step) for launch k of the slot, less the sampling / bootstrap arguments:
        launch k writes state k -- the frame stack of state k-1 and the frame ``fr`` env step k-1 returned, restarted where
        ``reset`` says; the bookmark for k == T -- and records env step k-1 (``rew``, ``done``); launch 0 copies the
        bookmark.  stash = (a1, a2, heads) rows of the update's buffers: the activations of state (slot, k) go there too."""
        D, T, S, slot0 = self.datas, c.T, c.S, c.slot0
        kw = dict(val_prev=c.val_prev.data_ptr(), rewards=D["rewards"].data_ptr(), dones=D["dones"].data_ptr(),
                  deltas=D["deltas"].data_ptr(), T=T, slot0=slot0, gamma=float(c.gamma), pong=int(c.pong))
        if stash is not None and k < T:      # conv activations of state (slot, k) -> row slot*T + k of the update's buffers
            n1, n2, hs = stash[0][0].numel(), stash[1][0].numel(), stash[2]
            kw.update(a1_out=stash[0].data_ptr() + 4 * (slot0 * T + k) * n1, a1_stride=T * n1,
                      a2_out=stash[1].data_ptr() + 4 * (slot0 * T + k) * n2, a2_stride=T * n2,
                      heads_out=hs.data_ptr() + 4 * (slot0 * T + k) * hs.stride(0), heads_out_stride=T * hs.stride(0))
        if k == 0:        # state of step 0 = the bookmark left by the previous slot (runner.py:190)
            kw.update(prev=c.bm.data_ptr(), prev_stride=S, out=c.sp(0), out_stride=T * S)
        else:
            out_ptr, out_stride = c.nxt(k - 1)
            kw.update(prev=c.sp(k - 1), prev_stride=T * S, reset_mask=reset.data_ptr(), out=out_ptr, out_stride=out_stride,
                      rew=rew.data_ptr(), done=done.data_ptr(), t_rec=k - 1)
            kw.update(dict(frame_u8=fr.ptr8, frame_stride=fr.stride) if fr.ptr8 else dict(frame_new=fr.ptr32))
        return kw

    def _rollout_block(self, net, slot0, env0, B, hyps):
        D, pool = self.datas, self.env_pool
        st = ops.stream()
        if hasattr(net, "_set_rollout_batch"):
            net._set_rollout_batch(B)
        net._refresh(st)
        for name in ("states", "rewards", "dones", "deltas") + (("truncs", "final_obs") if self.trunc else ()):
            ops._chk(D[name], name)
        c = _Slot(self, net, slot0, env0, B, hyps)
        self._stash_used = False
        if self._zero_copy_ok(net):
            return self._rollout_block_persistent(net, slot0, env0, B, hyps, c.bm, c.val_prev, c.acts_host_out, st)
        if not self.device_pool and os.environ.get("A2C_NO_STEP_GRAPHS") != "1":
            return self._rollout_block_segmented(c)
        if (self.device_pool and hasattr(pool, "device_step_post") and (not self.cont or self.float_pool)
                and c.acts_host_out is None and try_key(hyps, "rollout_graphs", True)
                and os.environ.get("A2C_NO_SLOT_GRAPH") != "1"):
            return self._rollout_block_device(c)
        self._fstore_ok = False          # this slot is played by a path that does not keep the frame store: it goes stale
        if c.h is None and getattr(net, "_step_supported", lambda: False)():
            return self._rollout_block_fused(c, st)
        # (The per-step bookkeeping launch only feeds later bookkeeping; running it on a second stream beside the frame-stack
        # launch was tried, and the fork and join cost more than they hid.)
        # state of step 0 = the bookmark left by the previous slot (runner.py:190)
        ops.copy_rows(c.bm.data_ptr(), c.S, c.sp(0), c.T * c.S, B, c.S, st)
        for t in range(c.T):
            a_ptr, a_stride = c.act_dst(t)
            vals = self._policy_step(c, t, a_ptr, a_stride, st)["vals"]
            fr, rew, done, reset = self._env_step(c, a_ptr, a_stride, t)
            self._post_step(c, t, fr, rew, done, reset, vals.data_ptr(), vals.stride(0),
                            os.environ.get("A2C_NO_POST_FUSE") != "1", st)
            self._norm_step(c, t, st)
        if self.bootstrap:
            self._bootstrap(c, st)

    def _post_step(self, c, t, fr, rew, done, reset, v_ptr, v_ld, fuse, st):
        """bookkeeping of env step t (runner.py:212-232; the values of state t are at v_ptr) and the next state
        (utils.next_state) into states[t+1], or into the bookmark after the last step.  fuse: feed-forward nets do both in
        ONE launch"""
        D, slot0, B, T, S, C, HW = self.datas, c.slot0, c.B, c.T, c.S, self.C, self.HW
        rewards, dones, deltas = D["rewards"], D["dones"], D["deltas"]
        nxt_ptr, nxt_stride = c.nxt(t)
        if fuse and c.h is None and HW % 4 == 0 and S % 4 == 0:
            if fr.ptr8:
                ops.rollout_post_u8(rew, done, v_ptr, v_ld, c.val_prev, rewards, dones, deltas, T, t, slot0, c.gamma, c.pong,
                                    fr.ptr8, fr.stride, reset, c.sp(t), T * S, nxt_ptr, nxt_stride, B, C, HW, st)
            else:
                ops.rollout_post(rew, done, v_ptr, v_ld, c.val_prev, rewards, dones, deltas, T, t, slot0, c.gamma, c.pong,
                                 _Ptr(fr.ptr32), reset, c.sp(t), T * S, nxt_ptr, nxt_stride, B, C, HW, st)
            return
        ops.rollout_record(rew, done, v_ptr, v_ld, c.val_prev, rewards, dones, deltas, c.done_eff, c.h, B, T, t, slot0,
                           c.gamma, c.pong, st)
        if fr.ptr8:
            ops.frame_stack_push_u8(fr.ptr8, fr.stride, reset, c.sp(t), T * S, nxt_ptr, nxt_stride, B, C, HW, st)
        else:
            ops.frame_stack_push(_Ptr(fr.ptr32), reset, c.sp(t), T * S, nxt_ptr, nxt_stride, B, C, HW, st)

    def _norm_step(self, c, t, st):
        """running normalisation of env step t, behind its post launch: the new plane of the next state
        and / or row t of the slots' rewards, ONE a2c_vecnorm_step; nothing without the keys.  Only enqueues"""
        n = self._norm
        if n is None:
            return
        D = self.datas
        nxt_ptr, nxt_stride = c.nxt(t)
        self.vecnorm.launch(c.B, c.env0, out_ptr=nxt_ptr if n["obs"] else 0, out_stride=nxt_stride, C=self.C,
                            rewards=D["rewards"] if n["rewards"] else None, dones=D["dones"] if n["rewards"] else None,
                            T=c.T, t=t, slot0=c.slot0, update=not self._norm_frozen, st=st)

    def _bootstrap(self, c, st):
        """bootstrap (runner.py:236-245): the value of the state after the last step closes the slot's deltas"""
        D = self.datas
        out = self._forward(c.net, c.bm.data_ptr(), c.S, c.B, c.env0, st)
        ops.rollout_bootstrap(out["vals"].data_ptr(), out["vals"].stride(0), c.val_prev, D["rewards"], D["dones"], D["deltas"],
                              c.B, c.T, c.slot0, c.gamma, st)

    def _rollout_block_fused(self, c, st, ub=None):
        """The same slot with ONE launch per step (a2c_a3c_step): launch t writes state t (frame
        stack of the frame env step t-1 returned), records env step t-1, runs the policy and samples
        action t; launch T records step T-1, leaves the bookmark and bootstraps (runner.py:174-248)."""
        net, env0, B, T = c.net, c.env0, c.B, c.T
        fr = rew = done = reset = None
        stash = self._stash_bufs
        self._stash_used = stash is not None
        for t in range(T + 1):
            kw = self._step_args(c, t, fr, rew, done, reset, stash)
            if t == T:
                net._step(B, st, bootstrap=int(self.bootstrap), **kw)
                break
            u = self._uniforms(t, B, env0) if ub is None else ub[t, env0:env0 + B]      # ub: the slot's persistent uniforms
            a_ptr, a_stride = c.act_dst(t)
            net._step(B, st, u=u.data_ptr(), actions=a_ptr, act_stride=a_stride, **kw)
            fr, rew, done, reset = self._env_step(c, a_ptr, a_stride, t)
            for name, x in (("rew", rew), ("done", done), ("reset", reset)):
                ops._chk(x, name)

    # ------------------------------------------------------------------ device pools: the slot as one hipGraph
    def _rollout_block_device(self, c):
        """Device env pools with ``device_step_post`` (the Snake / Pong / Breakout worlds): nothing happens on the host between
        the env steps, so the WHOLE slot -- T steps and the bootstrap -- is ONE hipGraph, like the relay branch of
        _rollout_block_segmented: the slot's noise lives in persistent buffers filled before the slot, outside the graph
        (``_slot_noise``); the first rollout of a key runs eagerly, the second is captured, later ones replay it; a failed
        capture issues the same launches eagerly, for good (``play_graph``).  Called with the stream already capturing (a
        caller's own graph), the block issues the same launches into that capture and leaves its warm / graph state alone.
        ``rollout_graphs=False`` (or A2C_NO_SLOT_GRAPH=1) is _rollout_block's eager loop, which plays the same steps bit
        for bit."""
        D, pool, net = self.datas, self.env_pool, c.net
        self._fstore_ok = False          # this slot does not keep the frame store: it goes stale
        ub = self._slot_noise(c.T, c.env0, c.B)
        fused = c.h is None and getattr(net, "_step_supported", lambda: False)()
        stash = self._stash_bufs if fused else None
        self._stash_used = stash is not None

        def body():
            st = ops.stream()      # (a capture runs on a stream of its own: not the one the caller was on)
            if fused:       # a2c_a3c_step records, stacks, runs the policy and samples; the world's plain step feeds it
                self._rollout_block_fused(c, st, ub=ub)
            else:
                self._device_slot(c, st, ub)
        if torch.cuda.is_current_stream_capturing():
            return body()
        stash_ptrs = None if stash is None else tuple(x.data_ptr() for x in stash if hasattr(x, "data_ptr"))
        # (the worlds' launches carry their env ids: a re-based pool is another key)
        key = (id(net), id(pool), int(getattr(pool, "env_id0", 0)), c.slot0, c.env0, c.B, c.T, float(c.gamma), c.pong, fused,
               stash_ptrs, tuple(D[k].data_ptr() for k in sorted(D) if D[k].is_cuda))
        if play_graph(self._dev_graphs, key, body) is False:      # capture not possible here: played eagerly from now on
            body()

    def _device_slot(self, c, st, ub):
        """the launches of one slot on a device pool, nets without the one-launch step kernel: per env step the policy step
        (``_policy_step``) and ONE launch for the world's step, the bookkeeping and the next state (a2c_<world>_step_post);
        then the bootstrap.  Only enqueues, reads its noise from the slot's persistent buffers: safe to capture."""
        D, pool, h = self.datas, self.env_pool, c.h
        slot0, env0, B, T, S = c.slot0, c.env0, c.B, c.T, c.S
        rewards, dones, deltas = D["rewards"], D["dones"], D["deltas"]
        ops.copy_rows(c.bm.data_ptr(), S, c.sp(0), T * S, B, S, st)      # state 0 = the bookmark (runner.py:190)
        for t in range(T):
            # (continuous nets: a2c_gauss_head writes the float action rows in place, from the slot's persistent noise)
            noise = (None, self._e_buf[t, env0:env0 + B]) if self.cont else (ub[t, env0:env0 + B], None)
            a_ptr, a_stride = c.act_row(t)
            vals = self._policy_step(c, t, a_ptr, a_stride, st, noise)["vals"]
            nxt_ptr, nxt_stride = c.nxt(t)
            # (done_eff is written for recurrent nets only, as the eager loop's a2c_rollout_record does)
            post = ops.world_post(vals.data_ptr(), vals.stride(0), c.val_prev, rewards, dones, deltas, T, t, slot0, c.gamma,
                                  c.pong, c.sp(t), T * S, nxt_ptr, nxt_stride, self.C,
                                  done_eff=None if h is None else c.done_eff, h=h)
            pool.device_step_post(t, env0, B, (a_ptr, a_stride), post, **(dict(trunc=c.trunc(t)) if self.trunc else {}))
            self._norm_step(c, t, st)
        if self.bootstrap:
            self._bootstrap(c, st)

    # ------------------------------------------------------------------ host pools: one hipGraph per time step
    def _rollout_block_segmented(self, c):
        """Host env pools (memcpy ingest): the slot is T+1 device SEGMENTS separated by the one host hand-off of
        each env step.  Segment k = [H2D of what env step k-1 returned + its bookkeeping + frame stack] followed by
        [forward + sampling of state k + D2H of the actions] (k < T) or by the bootstrap (k == T).  A segment has
        no host dependency inside, so each one is captured into a hipGraph the second time it runs (all pointers --
        rollout buffer rows, workspaces, the pinned pool region, the slot's noise buffers -- are stable across
        epochs) and replayed afterwards: ONE launch per env step instead of 5-30 (runner.py:198-232 per step)."""
        D, pool = self.datas, self.env_pool
        net, slot0, env0, B, T, hyps, h, acts_host_out = c.net, c.slot0, c.env0, c.B, c.T, c.hyps, c.h, c.acts_host_out
        dev = net._dev
        c.ub = self._slot_noise(T, env0, B)
        # device relay (a2c_pool_publish_actions / a2c_pool_ingest): the segments hand actions and frames to the env
        # workers through the pinned region themselves, so the T+1 launches queue back to back with no host in between
        relay = (self.proc_pool and pool.dev_ptr != 0 and acts_host_out is None and self.ingest != "memcpy"
                 and self.fstride % 16 == 0 and os.environ.get("A2C_NO_RELAY") != "1")
        if self.ingest == "relay" and not relay:
            raise ValueError("ingest='relay' needs a registered process/thread env pool and a device-resident "
                             "datas['actions'] tensor")
        if relay:
            if self._seq_dev is None:
                self._seq_dev = torch.zeros(1, dtype=torch.int32, device=dev)
                self._seq_pin = torch.zeros(64, dtype=torch.int32).pin_memory()      # ring: one entry per block in flight
                self._seq_i = 0
            i = self._seq_i % 64
            if i == 0 and self._seq_i:
                torch.cuda.current_stream().synchronize()       # the ring wraps: every earlier copy has been consumed
            self._seq_i += 1
            s32 = pool.seq_of(env0, B) & 0xffffffff               # the granules carry the step number modulo 2^32
            self._seq_pin[i] = s32 - (1 << 32) if s32 >= (1 << 31) else s32
            self._seq_dev.copy_(self._seq_pin[i:i + 1], non_blocking=True)
        stash = self._stash_bufs
        fused = h is None and getattr(net, "_step_supported", lambda: False)()
        if stash is not None and isinstance(stash, list) == fused:      # tuple (a1, a2): step kernel; list: conv-stack nets
            stash = None
        self._stash_used = stash is not None
        # Single-frame uint8 store (opt-in hyps['frame_store']): the ingest writes each new frame
        # straight into frames[slot][k+3], the first conv layer stacks its 4 planes on load, the fp32 `states` rows are
        # expanded from the store (per step, or on demand with hyps['lazy_states']) -- conv-stack nets behind the relay
        fs = None
        if relay and not fused and self.u8 and self.C == 4 and getattr(net, "_cl", None) and net._cl[0].frames_ok:
            fs = self._frame_store(T, D["states"].shape[0] // T, dev)
        if fs is None:
            self._fstore_ok = False      # this slot does not keep the store: it goes stale
        lazy = fs is not None and bool(try_key(hyps, "lazy_states", False))
        c.fused, c.stash, c.relay, c.fs, c.lazy = fused, stash, relay, fs, lazy
        if fs is not None:
            if self._stash_used:
                self._frames_written = (fs[0], fs[1], T)
            if lazy:
                self._states_stale = True
                net._materialize_states = self.materialize_states

        def whole():
            for k in range(T + 1):
                self._segment(k, c)
        cache = key = None
        if try_key(hyps, "rollout_graphs", True) and torch.cuda.is_available():
            cache = self._seg_graphs
            key = (id(net), slot0, env0, B, T, fused, stash is not None, acts_host_out is None, c.pong, relay, float(c.gamma),
                   fs is not None, lazy, tuple(D[k].data_ptr() for k in sorted(D) if D[k].is_cuda))
        if cache is not None and relay and os.environ.get("A2C_NO_SLOT_GRAPH") != "1":
            # device relay: nothing happens on the host between the segments, so the WHOLE slot (T+1 segments, a few
            # thousand kernel nodes) is ONE hipGraph; a failed capture falls back to one graph per segment
            if play_graph(cache, key + ("slot",), whole) is not False:
                self._mark_cells_done(c)
                return
        for k in range(T + 1):
            # (a segment whose capture failed is played eagerly)
            if cache is None or play_graph(cache, key + (k,), lambda: self._segment(k, c)) is False:
                self._segment(k, c)
            if k < T and not relay:     # the host hand-off of env step k
                torch.cuda.current_stream().synchronize()
                self._host_env_step(c, k)
        self._mark_cells_done(c)

    def _mark_cells_done(self, c):
        ro = getattr(c.net, "_roll_outputs", None)
        if ro and c.stash is not None and c.fused_post and ro((c.stash, c.slot0 * c.T, c.T), c.B) is not None:
            c.net._cells_done = c.T - 1      # every step of every slot went through the cell stash (eagerly or replayed)

    def _values_src(self, c, k):
        """-> (v_ptr, v_ld, h_src): where segment k - 1's forward left the values of its states and its new hidden rows -- the
        roll buffers (h_src 0: ``h`` itself), or rows of the update's buffers (GRUModel's cell stash, which needs the fused post
        kernels) -- a pure function of (net, k), safe under graph replay"""
        hb, logits, vals = c.net._heads("roll", c.B)
        ro = getattr(c.net, "_roll_outputs", None)
        prev = None
        if ro and c.stash is not None and k > 0 and c.fused_post:
            prev = ro((c.stash, c.slot0 * c.T + k - 1, c.T), c.B)
        return prev if prev else (vals.data_ptr(), vals.stride(0), 0)

    def _post_frames_args(self, k, c):
        """arguments of a2c_rollout_post_frames for env step k - 1 of this slot (after rew, done; before the stream)"""
        D, h = self.datas, c.h
        v_ptr, v_ld, h_src = self._values_src(c, k)
        F_, nv_rows, nv_carry = c.fs
        hrow = hstride = 0
        if h is not None:
            hrow, hstride = c.h_row(k) if k < c.T else (0, c.T * h.shape[1])
        return (v_ptr, v_ld, c.val_prev, D["rewards"], D["dones"], D["deltas"], c.T, k - 1, c.slot0, c.gamma, c.pong,
                c.done_eff, h, hrow, hstride, h_src, nv_rows, nv_carry.data_ptr() + 4 * c.env0)

    def _segment(self, k, c):
        """device work of segment k (see _rollout_block_segmented); only enqueues, never waits on the host"""
        net, slot0, env0, B, T, hyps = c.net, c.slot0, c.env0, c.B, c.T, c.hyps
        D, pool, S, C, HW = self.datas, self.env_pool, self.S, self.C, self.HW
        sp, bm, val_prev, done_eff, h = c.sp, c.bm, c.val_prev, c.done_eff, c.h
        gamma, pong = c.gamma, c.pong
        rewards, dones, deltas = D["rewards"], D["dones"], D["deltas"]
        st = ops.stream()
        fr = rew = done = None
        if k > 0 and c.relay:       # what env step k-1 returned: waited for and fetched by the device itself
            rew, done = self.d_rew[env0:env0 + B], self.d_done[env0:env0 + B]
            fs, ds = self.fstride, self.dstride
            dst = self.d_frames.data_ptr() + env0 * ds
            if c.fs is not None:      # single-frame store: the new frame lands in frames[slot][k+3], nowhere else
                F_ = c.fs[0]
                ds = F_.stride(0)
                dst = F_.data_ptr() + slot0 * ds + (k + 3) * HW
            ticks = int(float(try_key(hyps, "env_timeout_s", 20.0)) * 1e8)
            post = None
            if c.fs is not None and not self.dev_prep and os.environ.get("A2C_NO_FUSED_POST_INGEST") != "1":
                post = self._post_frames_args(k, c)
            if post is not None:     # the ingest workgroup of an env also does its bookkeeping (rollout_post_frames) of step k - 1
                ops.pool_ingest_post(self.bits, pool.dev_rec + 8 * env0, pool.dev_frames + env0 * fs, fs, HW if self.bits else fs, B,
                                     self._seq_dev, k, ticks, self.rollout_err, rew, done, dst, ds, *post, st)
                c.post_done = k
            elif self.dev_prep:      # raw frames cross the link; crop / stride / binarise on the device into dst
                raw = self.d_raw.data_ptr() + env0 * fs
                ops.pool_ingest(pool.dev_rec + 8 * env0, pool.dev_frames + env0 * fs, fs, fs, B, self._seq_dev, k,
                                ticks, self.rollout_err, rew, done, raw, fs, st)
                ops.frame_prep_u8(self.dev_prep, raw, fs, *self.raw_dims, dst, ds, B, st)
            elif self.bits:
                ops.pool_ingest_bits(pool.dev_rec + 8 * env0, pool.dev_frames + env0 * fs, fs, HW, B, self._seq_dev, k,
                                     ticks, self.rollout_err, rew, done, dst, ds, st)
            else:
                ops.pool_ingest(pool.dev_rec + 8 * env0, pool.dev_frames + env0 * fs, fs, fs, B, self._seq_dev, k,
                                ticks, self.rollout_err, rew, done, dst, ds, st)
            fr = self._staged_frames(dst, env0, B, st) if c.fs is None else None
        elif k > 0:     # what env step k-1 returned: pinned staging -> HBM
            rew, done = self.d_rew[env0:env0 + B], self.d_done[env0:env0 + B]
            rew.copy_(self.h_rew[env0:env0 + B], non_blocking=True)
            done.copy_(self.h_done[env0:env0 + B], non_blocking=True)
            if self.proc_pool:
                fr = self._pool_frames_h2d(pool, env0, B, st)
            else:
                df = self.d_frames[env0:env0 + B]
                df.copy_(self.h_frames[env0:env0 + B], non_blocking=True)
                fr = _Frames(ptr32=df.data_ptr())
        act = c.act
        a_ptr, a_stride = c.act_dst(min(k, T - 1))
        if c.fused:      # a2c_a3c_step: record(k-1) + frame stack + forward + sample (+ bootstrap) in ONE launch
            kw = self._step_args(c, k, fr, rew, done, done, c.stash)      # (a host pool's envs reset where they are done)
            if k == T:
                net._step(B, st, bootstrap=1, **kw)
                return
            net._step(B, st, u=c.ub[k, env0:env0 + B].data_ptr(), actions=a_ptr, act_stride=a_stride, **kw)
        else:
            fused_post = c.fused_post
            v_ptr, v_ld, h_src = self._values_src(c, k)
            h_row_done = False
            if c.fs is not None:
                F_, nv_rows, nv_carry = c.fs
                ss = F_.stride(0)
                f0 = F_.data_ptr() + slot0 * ss
                nvr, nvc = nv_rows.data_ptr() + 4 * slot0 * T, nv_carry.data_ptr() + 4 * env0
                if k == 0:  # state 0 = the window the previous slot ended with (the bookmark, runner.py:190)
                    ops.frame_store_begin(f0, ss, T, C, HW, nvr, nvc, B, st)
                elif c.post_done == k:      # ... done by the ingest launch of this segment (a2c_pool_ingest_post)
                    h_row_done = h is not None
                else:       # bookkeeping of env step k-1 (runner.py:212-232); the frame is already in the store
                    pa = self._post_frames_args(k, c)
                    ops.rollout_post_frames(rew, done, *pa[:11], B, *pa[11:], st)
                    h_row_done = h is not None
                if k == T:  # the bookmark state stays materialised: any other rollout path can take over from here
                    ops.frames_to_states(f0 + T * HW, ss, nvc, 1, bm.data_ptr(), S, B, 1, C, HW, st)
                    net._frames_src = (f0 + T * HW, ss, 1, nvc, 1)
                else:
                    if not c.lazy:   # the reference's fp32 row of `states` (runner.py:199), expanded from the window
                        ops.frames_to_states(f0 + k * HW, ss, nvr + 4 * k, T, sp(k), T * S, B, 1, C, HW, st)
                    net._frames_src = (f0 + k * HW, ss, 1, nvr + 4 * k, T)
            elif k == 0:    # state of step 0 = the bookmark left by the previous slot (runner.py:190)
                ops.copy_rows(bm.data_ptr(), S, sp(0), T * S, B, S, st)
            else:           # bookkeeping of env step k-1 + the next state (utils.next_state)
                t = k - 1
                if fused_post:
                    # recurrent nets: bookkeeping + frame stack + hidden-state reset + the h_states row in ONE launch
                    nxt_ptr, nxt_stride = c.nxt(t)
                    hrow = c.h_row(k)[0] if k < T else 0
                    ops.rollout_post_rec(rew, done, v_ptr, v_ld, val_prev, rewards, dones, deltas, T, t,
                                         slot0, gamma, pong, fr.ptr32 or 0, fr.ptr8 or 0, fr.stride if fr.ptr8 else 0, done,
                                         sp(t), T * S, nxt_ptr, nxt_stride, B, C, HW, done_eff, h, hrow, T * h.shape[1],
                                         h_src_ptr=h_src, st=st)
                    h_row_done = True
                else:       # (a host pool's envs reset where they are done)
                    self._post_step(c, t, fr, rew, done, done, v_ptr, v_ld, True, st)
            if k == T:
                try:
                    self._bootstrap(c, st)
                finally:
                    net._frames_src = None
                return
            if h is not None and not h_row_done:                            # h_states[e] = h (runner.py:201)
                ops.copy_rows(h.data_ptr(), h.shape[1], *c.h_row(k), B, h.shape[1], st)
            u = c.ub[k, env0:env0 + B]
            net._cell_stash_ok = fused_post            # the cell stash needs the fused post kernel (h_src) of the next segment
            try:
                pub = None      # device relay: the heads kernel's sampling thread hands the action to the env worker itself
                if c.relay and os.environ.get("A2C_NO_FUSED_PUBLISH") != "1":
                    pub = (pool.dev_cmd + 8 * env0, self._seq_dev, k)
                out = self._forward(net, sp(k), T * S, B, env0, st, sampler=(u, a_ptr, a_stride, pub),
                                    stash=None if c.stash is None else (c.stash, slot0 * T + k, T))
            finally:
                net._frames_src = None
            if not out.get("sampled", False):
                gpub = None
                if c.relay and self.cont:      # float action granules + doorbells of env step k, from the sampling threads
                    ast = int(pool.header.act_stride)
                    gpub = (pool.dev_act + 8 * ast * env0, ast, pool.dev_cmd + 8 * env0, self._seq_dev, k)
                self._sample(net, out["logits"], u, self._e_buf[k, env0:env0 + B] if self.cont else None, a_ptr, a_stride,
                             B, st, pub=gpub)
                if gpub is not None:
                    out["published"] = True
            if out.get("h_next_src") is not None:      # cell stash: the next segment's post kernel reads h_new from there
                pass
            elif h is not None and out["h"].data_ptr() != h.data_ptr():    # (the GRU models update h in place)
                ops.copy_rows(out["h"].data_ptr(), h.shape[1], h.data_ptr(), h.shape[1], B, h.shape[1], st)
        if c.relay:      # the sampled actions go to the env workers: cmd granules of env step k
            if not c.fused and out.get("published", False):
                return
            ops.pool_publish_actions(pool.dev_cmd + 8 * env0, a_ptr, a_stride, B, self._seq_dev, k, st)
            return
        # the sampled actions go to the host (pinned staging) at the tail of the segment
        ha = self.h_act[env0:env0 + B]
        if (a_ptr == act.data_ptr()) if self.cont else a_stride == 1:
            ha.copy_(act, non_blocking=True)
        else:
            if self._act_gather is None:
                self._act_gather = torch.zeros_like(self.act_dev)
            ag = self._act_gather[env0:env0 + B]
            ag.copy_(D["actions"][slot0 * T + k::T][:B])
            ha.copy_(ag, non_blocking=True)

    def _pool_exchange(self, c, t):
        """process pool: the actions of env step t (pinned staging) go to the workers, which step their envs in parallel;
        wait for them; their rewards / dones come into the pinned staging (the frames stay in the pool's region)"""
        pool, env0, B = self.env_pool, c.env0, c.B
        k = pool.seq_of(env0, B) + t
        pool.post_actions(self.np_act[env0:env0 + B], env0=env0, seq=k)
        c.acts_to_host_out(t, self.h_act[env0:env0 + B])
        pool.wait_frames(k + 1, env0=env0, n=B, timeout=float(try_key(self.hyps, "env_timeout_s", 20.0)))
        pool.unpack(self.np_rew[env0:env0 + B], self.np_done[env0:env0 + B], env0=env0)

    def _host_env_step(self, c, t):
        """host half of env step t (the D2H of the actions has completed): hand the actions to the envs, wait for them,
        leave rewards / dones (/ frames) in the pinned staging that is copied up next"""
        if self.proc_pool:
            return self._pool_exchange(c, t)
        host_env_step(self.env_pool, c.env0, c.B, self.np_act, self.np_frames, self.np_rew, self.np_done, self.ep_rew,
                      self.rew_q, c.shift, c.pong, self.cont)
        c.acts_to_host_out(t, self.h_act[c.env0:c.env0 + c.B])

    def _rollout_block_persistent(self, net, slot0, env0, B, hyps, bm, val_prev, acts_host_out, st):
        """The whole slot as ONE persistent launch (a2c_a3c_rollout): the workgroups and the env worker
        processes hand actions and uint8 frames to each other through the pinned pool region; nothing
        runs on the host of this process until the launch has finished."""
        D, pool = self.datas, self.env_pool
        T, S = int(hyps["n_tsteps"]), self.S
        dev = net._dev
        if self.uniform_fn is not None:
            u = torch.stack([self.uniform_fn(t, B, env0).reshape(B) for t in range(T)]).contiguous()
        else:
            u = torch.rand((T, B), device=dev, dtype=torch.float32)
        ops._chk(u, "uniforms")
        if acts_host_out is None:
            acts = D["actions"]
        else:
            if self._acts_dev is None or self._acts_dev.numel() != D["actions"].numel():
                self._acts_dev = torch.zeros(D["actions"].numel(), dtype=torch.int64, device=dev)
            acts = self._acts_dev
        C, H, W = net.input_space[-3:]
        hb, _, _ = net._heads("roll", self.B)
        hb = hb[env0:env0 + B]
        P = net.P
        self._u_keep = u          # stays alive until the launch has consumed it
        timeout_s = float(try_key(hyps, "env_timeout_s", 20.0))
        # single-frame uint8 store (row f4): T+4 frames per slot, created with the bookmark in start(); the update's
        # first-layer weight gradient stacks the frames on load instead of reading the 4x duplicated fp32 states
        fs = self._frame_store(T, D["states"].shape[0] // T, dev)
        # only the ring kernel can leave the fp32 rows out (more envs than CUs: interleaved blocks of it, one after the
        # other); the library answers whether THIS call runs it (LDS budget, conv1 output size, weight alignment,
        # A2C_NO_RING / A2C_RING_BLOCKS) -- a shape that does not gets its rows written by the per-step body instead
        ring = ops.a3c_ring_supported(B, C, H, W, net.output_space, P("convs.0.0.weight").data_ptr())
        lazy = fs is not None and bool(try_key(hyps, "lazy_states", False)) and ring
        # ... and only the ring kernel writes the lane masks of the a1 stash rows (the update's conv2 backward-data mask)
        lm = self._stash_bufs[3] if (ring and self._stash_bufs is not None and len(self._stash_bufs) > 3) else None
        mb = self._stash_bufs[4] if (lm is not None and len(self._stash_bufs) > 4) else None
        ops.a3c_rollout(st, B=B, C=C, H=H, W=W, n_actions=net.output_space, states=D["states"].data_ptr(),
                        bookmark=bm.data_ptr(), wfrag1=net._c1.wf.data_ptr(), bias1=P("convs.0.0.bias").data_ptr(),
                        wfrag2=net._c2.wf.data_ptr(), bias2=P("convs.1.0.bias").data_ptr(), Wc=net._Wc.data_ptr(),
                        bc=net._bc.data_ptr(), heads=hb.data_ptr(), ldh=hb.stride(0), u=u.data_ptr(), u_stride=B,
                        actions=acts.data_ptr(), val_prev=val_prev.data_ptr(), rewards=D["rewards"].data_ptr(),
                        dones=D["dones"].data_ptr(), deltas=D["deltas"].data_ptr(), T=T, slot0=slot0,
                        gamma=float(hyps["gamma"]), pong=int("Pong" in hyps["env_type"]), cmd=pool.dev_cmd, rec=pool.dev_rec,
                        frames=pool.dev_frames, frame_stride=self.fstride, frame_bits=int(self.bits),
                        conv1_weight=P("convs.0.0.weight").data_ptr(),
                        seq0=pool.seq_of(env0, B) & 0xffffffff, env0=env0,
                        err=self.rollout_err.data_ptr(), timeout_ticks=int(timeout_s * 1e8),
                        a1_rows=0 if self._stash_bufs is None else self._stash_bufs[0].data_ptr(),
                        a2_rows=0 if self._stash_bufs is None else self._stash_bufs[1].data_ptr(),
                        heads_rows=0 if self._stash_bufs is None else self._stash_bufs[2].data_ptr(),
                        heads_rows_ld=0 if self._stash_bufs is None else self._stash_bufs[2].stride(0),
                        frame_store=0 if fs is None else fs[0].data_ptr(),
                        frame_store_slot_stride=0 if fs is None else fs[0].stride(0),
                        nvalid_rows=0 if fs is None else fs[1].data_ptr(),
                        nvalid_carry=0 if fs is None else fs[2][env0:env0 + B].data_ptr(), states_lazy=int(lazy),
                        tagged=getattr(pool, "dev_tagged", 0), tagged_stride=int(pool.header.tagged_stride),
                        tagged_chunks=int(pool.header.tagged_chunks), a1_lanemask_rows=0 if lm is None else lm.data_ptr(),
                        a2_maskbit_rows=0 if mb is None else mb.data_ptr())
        # every block of the call must have written them (a rollout of several blocks: all ring launches, or none counts)
        self._lm_written = (lm is not None) and (self._lm_written or slot0 == 0)
        if lazy:            # (only after the launch was accepted: a refused call must not leave rows marked stale)
            self._states_stale = True
            net._materialize_states = self.materialize_states
        if fs is not None and self._stash_bufs is not None:
            self._frames_written = (fs[0], fs[1], T)
        self._stash_used = self._stash_bufs is not None
        if acts_host_out is not None:
            acts_host_out[slot0 * T:(slot0 + B) * T].copy_(acts[slot0 * T:(slot0 + B) * T])

    def materialize_states(self):
        """hyps['lazy_states']: the rollout kept one uint8 frame per env step (+ valid-plane counts) and did not write the
        fp32 ``states`` rows; this expands ALL of them (runner.py:199's layout and values, bit for bit) -- called by the
        net when an update needs the rows (no activation stash), by ``finish()`` unless hyps['lazy_states'], or by hand."""
        if not self._states_stale:
            return
        F_, nv_rows, _ = self._fstore
        R, T = F_.shape[0], F_.shape[1] - 4
        st = self.datas["states"]
        ops.frames_to_states(F_.data_ptr(), F_.stride(0), nv_rows.data_ptr(), T, st.data_ptr(), T * self.S, R, T, self.C, self.HW)
        self._states_stale = False

    def _frame_store(self, T, R, dev):
        """(frames uint8 (R, T+4, HW), nvalid_rows int32 (R*T,), nvalid_carry int32 (B,)) or None.  OPT-IN
        (hyps['frame_store'] / A2C_FRAME_STORE=1): on MI355X the first-layer weight gradient is matrix-bound, not
        HBM-bound, and runs 10 % SLOWER from the uint8 store (1.41 vs 1.27 ms at N = 32 768: the uint8 -> fp32
        expansion sits in the commit phase all waves wait on) although it reads 4x fewer bytes.  Valid only while
        EVERY env step since start() went through the persistent kernel (it is the only writer): the first slot finds
        frames[:, T+3] = the reset frame and one valid plane; any other rollout path switches the store off.
        The store is four planes deep (T + 4 frames per slot, valid-plane counts saturating at 4 in
        a2c_rollout_post_frames): any other n_frame_stack keeps the fp32 states."""
        on = os.environ.get("A2C_FRAME_STORE") == "1" or bool(try_key(self.hyps, "frame_store", False))
        if not on or os.environ.get("A2C_NO_FRAME_STORE") == "1" or T < 4 or self.HW % 16 or self.C != 4 or \
                not self._fstore_ok:
            return None
        fs = self._fstore
        if fs is None:
            if (self.env_pool.seq_env != self.env_pool.seq_start).any() or R != self.B:
                self._fstore_ok = False
                return None
            F_ = torch.zeros((R, T + 4, self.HW), dtype=torch.uint8, device=dev)
            F_[:, T + 3] = self.d_frames[:, :self.HW]          # frame 0 of every env (its env.reset()), still in HBM from start()
            fs = self._fstore = (F_, torch.zeros(R * T, dtype=torch.int32, device=dev),
                                 torch.ones(self.B, dtype=torch.int32, device=dev))
        return fs

    # ------------------------------------------------------------------ one env step of B envs
    def _env_step(self, c, a_ptr, a_stride, t):
        """-> (_Frames, rew, done, reset) device views of what the envs returned for the actions just sampled"""
        pool, env0, B = self.env_pool, c.env0, c.B
        if self.device_pool:
            if getattr(pool, "needs_actions", False):      # an action-driven world: where the sampler wrote this step's actions
                kw = dict(trunc=c.trunc(t)) if self.trunc else {}
                frames, rew, done, reset = pool.device_step(t, env0, B, actions=(a_ptr, a_stride), **kw)
                if c.acts_host_out is not None:            # a host `actions` tensor like the reference's: one D2H per step
                    c.acts_to_host_out(t, c.act.cpu())
            else:
                frames, rew, done, reset = pool.device_step(t, env0, B)
            ops._chk(frames, "frames")
            return _Frames(ptr32=frames.data_ptr()), rew, done, reset
        if self.proc_pool:
            return self._pool_step(c, a_stride, t)
        return self._host_step(c, a_stride, t)

    def _actions_to_host(self, c, a_stride, t):
        ha = self.h_act[c.env0:c.env0 + c.B]
        if (not self.datas["actions"].is_cuda) if self.cont else a_stride == 1:
            ha.copy_(c.act, non_blocking=True)
        else:
            ha.copy_(self.datas["actions"][c.slot0 * c.T + t::c.T][:c.B], non_blocking=True)
        torch.cuda.current_stream().synchronize()

    def _staged_frames(self, dst, env0, B, st):
        """_Frames of the B frames staged at ``dst`` (stride self.dstride): uint8 pixels, or fp32 (compacted to dense
        rows first when the pool's slots are padded: frame sizes that are not a multiple of 16 B)"""
        if self.u8:
            return _Frames(ptr8=dst, stride=self.dstride)
        if self.d_dense is None:
            return _Frames(ptr32=dst)
        dense = self.d_dense.data_ptr() + 4 * env0 * self.HW
        ops.copy_rows(dst, self.dstride // 4, dense, self.HW, B, self.HW, st)
        return _Frames(ptr32=dense)

    def _pool_frames_h2d(self, pool, env0, B, st):
        """hipMemcpyAsync of the frames block of envs env0..env0+B from the pinned region into HBM"""
        fs, ds = self.fstride, self.dstride
        dst = self.d_frames.data_ptr() + env0 * ds
        src = pool.region.base + pool.header.off_frames + env0 * fs
        if self.dev_prep:
            raw = self.d_raw.data_ptr() + env0 * fs
            ops.memcpy_async(raw, src, B * fs, ops.H2D, st)
            ops.frame_prep_u8(self.dev_prep, raw, fs, *self.raw_dims, dst, ds, B, st)
        elif self.bits:     # the packed slots cross the link, one kernel expands them to the uint8 pixels the step kernels read
            pk = self.d_packed.data_ptr() + env0 * fs
            ops.memcpy_async(pk, src, B * fs, ops.H2D, st)
            ops.unpack_bits(pk, fs, dst, ds, B, self.HW, st)
        else:
            ops.memcpy_async(dst, src, B * fs, ops.H2D, st)
        return self._staged_frames(dst, env0, B, st)

    def _pool_step(self, c, a_stride, t):
        """memcpy ingest with the process pool: actions D2H -> the workers step their envs in parallel ->
        frames H2D from the pinned region (uint8 when the pool carries uint8) + rewards / dones."""
        env0, B = c.env0, c.B
        self._actions_to_host(c, a_stride, t)
        self._pool_exchange(c, t)
        fr = self._pool_frames_h2d(self.env_pool, env0, B, ops.stream())
        dr, dd = self.d_rew[env0:env0 + B], self.d_done[env0:env0 + B]
        dr.copy_(self.h_rew[env0:env0 + B], non_blocking=True)
        dd.copy_(self.h_done[env0:env0 + B], non_blocking=True)
        return fr, dr, dd, dd

    def _host_step(self, c, a_stride, t):
        """serial in-process pool: actions D2H -> env.step one after the other -> frames/rewards/dones H2D
        through pinned buffers (numpy views of them: no per-element tensor writes)."""
        env0, B = c.env0, c.B
        self._actions_to_host(c, a_stride, t)
        self._host_env_step(c, t)
        df, dr, dd = (x[env0:env0 + B] for x in (self.d_frames, self.d_rew, self.d_done))
        df.copy_(self.h_frames[env0:env0 + B], non_blocking=True)
        dr.copy_(self.h_rew[env0:env0 + B], non_blocking=True)
        dd.copy_(self.h_done[env0:env0 + B], non_blocking=True)
        return _Frames(ptr32=df.data_ptr()), dr, dd, dd


class _Ptr:
    """raw device address with the ``data_ptr()`` the ops wrappers ask for"""
    __slots__ = ("p",)

    def __init__(self, p):
        self.p = int(p)

    def data_ptr(self):
        return self.p


class StatsRunner:
    """Evaluation rollouts (runner.py:250-314) with the training sampler.

    The reference plays ``n_test_eps`` episodes of ONE env one after the other with batch-1 forwards on the main
    process, every epoch (training.py:167) -- with a millisecond-scale update that serial loop would dominate
    ``train()``.  Here the ``n_test_eps`` episodes are played by ``n_test_eps`` envs in LOCK-STEP: one batched
    forward + sampling launch per step for all of them (the one-launch step kernel for A3CModel-shaped nets),
    each env plays exactly one episode and the result is (sum of the episode rewards) / n_test_eps -- the same
    estimator over the same number of episodes.  ``StatsRunner(hyps, env=one_env)`` keeps the reference's serial
    loop (same episodes in the same order as the reference) for callers that own a single env object."""

    def __init__(self, hyps, env=None, envs=None, uniform_fn=None, normal_fn=None, norm=None):
        self.hyps = hyps
        # norm: the training Runner's DeviceVecNorm (or a callable that returns it) under hyps norm_obs: every observation is
        # normalised by its moments as they stand when the evaluation begins (one snapshot() per rollout), frozen
        self.norm = norm
        if bool(try_key(hyps, "norm_obs", False)) and (norm is None or (env is not None and envs is None)):
            raise ValueError("norm_obs: StatsRunner normalises the observations of lock-step host twins (envs=...) by the "
                             "training Runner's block: pass norm=runner.vecnorm")
        self.n_episodes = try_key(hyps, "n_test_eps", 15)
        self.uniform_fn = uniform_fn              # (t, E) -> (E,) device uniforms; default torch.rand
        self.normal_fn = normal_fn                # continuous nets: (t, E, 0) -> (E, n) device N(0,1); default torch.randn
        self.obs_deque = deque(maxlen=hyps["n_frame_stack"])
        self.envs = list(envs) if envs is not None else None
        self.env = env
        if env is None and envs is None:
            seed = try_key(hyps, "seed", 0)
            self.envs = [SequentialEnvironment(**dict({k: v for k, v in hyps.items() if k != "seed"}, seed=seed + 10007 + j))
                         for j in range(self.n_episodes)]
            self.env = self.envs[0]               # the reference's attribute (training.py:61 reads stats_runner.env)

    def rollout(self, net):
        if self.envs is None:
            return self._rollout_serial(net)
        return self._rollout_batched(net)

    # ---- E envs, one episode each, in lock-step on the device
    def _rollout_batched(self, net, max_steps=None):
        hyps, envs = self.hyps, self.envs
        E = len(envs)
        net._ensure_device()
        dev = net._dev
        st = ops.stream()
        net._refresh(st)
        C = int(hyps["n_frame_stack"])
        shift, pong = hyps["action_shift"], "Pong" in hyps["env_type"]
        snap = None
        if self.norm is not None and bool(try_key(hyps, "norm_obs", False)):
            snap = (self.norm() if callable(self.norm) else self.norm).snapshot()
        prep = (lambda o: np.asarray(o, dtype=np.float32)) if snap is None else \
            (lambda o: snap.normalize_obs(np.asarray(o, dtype=np.float32).reshape(-1)))
        first = [prep(e.reset()) for e in envs]
        HW = first[0].size
        S = C * HW
        pin = torch.cuda.is_available()
        h_frames = torch.zeros(E, HW).pin_memory() if pin else torch.zeros(E, HW)
        np_frames = h_frames.numpy()
        for j in range(E):
            np_frames[j] = first[j].reshape(-1)
        f32 = dict(dtype=torch.float32, device=dev)
        d_frames = torch.zeros(E, HW, **f32)
        cur, nxt = torch.zeros(E, S, **f32), torch.zeros(E, S, **f32)
        ones, zeros = torch.ones(E, **f32), torch.zeros(E, **f32)
        cont, n = not getattr(net, "is_discrete", True), int(net.output_space)
        act_dev = torch.zeros((E, n), **f32) if cont else torch.zeros(E, dtype=torch.int64, device=dev)
        h = torch.zeros(E, net.h_size, **f32) if net.is_recurrent else None
        d_frames.copy_(h_frames, non_blocking=True)
        ops.frame_stack_push(d_frames, ones, cur.data_ptr(), S, cur.data_ptr(), S, E, C, HW, st)      # [0,..,0, env.reset()]
        fused = (not net.is_recurrent) and getattr(net, "_step_supported", lambda: False)()
        active = np.ones(E, dtype=bool)
        ep_rew = np.zeros(E)
        t = 0
        max_steps = max_steps or int(try_key(hyps, "max_eval_steps", 10 ** 6))
        while active.any() and t < max_steps:
            if cont:
                eps = self.normal_fn(t, E, 0).reshape(E, n) if self.normal_fn is not None else torch.randn((E, n), **f32)
            else:
                u = self.uniform_fn(t, E) if self.uniform_fn is not None else torch.rand(E, **f32)
            if fused:       # state t = push(state t-1, frame) + forward + sample in ONE launch
                kw = dict(prev=cur.data_ptr(), prev_stride=S) if t == 0 else \
                    dict(prev=cur.data_ptr(), prev_stride=S, frame_new=d_frames.data_ptr(), reset_mask=zeros.data_ptr(),
                         out=nxt.data_ptr(), out_stride=S)
                net._step(E, st, u=u.data_ptr(), actions=act_dev.data_ptr(), act_stride=1, **kw)
                if t > 0:
                    cur, nxt = nxt, cur
            else:
                if t > 0:
                    ops.frame_stack_push(d_frames, zeros, cur.data_ptr(), S, nxt.data_ptr(), S, E, C, HW, st)
                    cur, nxt = nxt, cur
                if net.is_recurrent:
                    out = net._fwd(cur.data_ptr(), S, E, "eval", st, False, h_in=h)
                else:
                    out = net._fwd(cur.data_ptr(), S, E, "eval", st, False, sampler=(u, act_dev.data_ptr(), 1)) \
                        if getattr(net, "_fused_sampling", False) else net._fwd(cur.data_ptr(), S, E, "eval", st, False)
                if cont:
                    ops.gauss_head(out["logits"], n, E, eps=eps, actions_ptr=act_dev.data_ptr(), act_ld=n, st=st)
                elif not out.get("sampled", False):
                    ops.softmax_sample(out["logits"], u, act_dev.data_ptr(), 1, E, net.output_space, st=st)
                if net.is_recurrent:
                    h.copy_(out["h"])
            acts = act_dev.cpu().numpy()                       # the one host round trip of the step
            for j in np.nonzero(active)[0]:
                obs, rew, done, _ = envs[j].step(acts[j] + np.float32(shift) if cont else int(acts[j]) + shift)
                ep_rew[j] += rew
                if pong and rew != 0:
                    done = True
                if done:                                        # this env's episode is over: it stops playing
                    active[j] = False
                else:
                    np_frames[j] = prep(obs).reshape(-1)
            d_frames.copy_(h_frames, non_blocking=True)
            t += 1
        return float(ep_rew.sum()) / E

    # ---- the reference's loop, one env, batch 1 (runner.py:274-314)
    def _rollout_serial(self, net):
        state = next_state(self.env, self.obs_deque, obs=None, reset=True)
        h = cuda_if(torch.zeros(1, net.h_size)) if net.is_recurrent else None
        ep_rew, ep_count = 0, 0
        with torch.no_grad():
            while ep_count < self.n_episodes:
                x = cuda_if(torch.FloatTensor(state))[None]
                if h is not None:
                    val, logits, h = net(x, h)
                else:
                    val, logits = net(x)
                action = self.env.get_action(logits)
                obs, rew, done, _ = self.env.step(action + self.hyps["action_shift"])
                ep_rew += rew
                reset = done
                if "Pong" in self.hyps["env_type"] and rew != 0:
                    done = True
                if done:
                    ep_count += 1
                    if h is not None:
                        h = cuda_if(torch.zeros(1, net.h_size))
                state = next_state(self.env, self.obs_deque, obs=obs, reset=reset)
        return ep_rew / ep_count


class DeviceStatsRunner:
    """``StatsRunner`` for the device-resident worlds (``snake.DeviceSnakePool``, ``pong.DevicePongPool``,
    ``breakout.DeviceBreakoutPool``): ``pool`` holds E = n_test_eps worlds, each plays exactly ONE episode per ``rollout(net)``
    and the result is (sum of the episode rewards) / E, as ``StatsRunner._rollout_batched`` -- with nothing on the host.

    There is no second rollout loop: a private ``Runner`` plays the E worlds in chunks of K = ``hyps['eval_chunk']`` (default
    32) lock-step steps with the launches of the training path (a chunk is one slot graph: first chunk of a call eager, second
    captured, later ones replayed), a2c_eval_scan closes every env at its first done out of the chunk's rewards / dones rows,
    and ONE 4-byte read per chunk tells the host whether an env is still playing.  ``hyps['max_eval_steps']`` (default 10**6)
    caps the episode; the cap may fall inside a chunk.  A step here is an AGENT step of the pool: on worlds with
    ``frame_skip`` = k > 1 ``last["ep_len"]`` and ``max_eval_steps`` count agent steps, up to k game frames each.

    Every call plays fresh, reproducible worlds: call c re-bases the pool to env ids 10007 + c*E .. (the first call: the
    ids of ``train()``'s host twins).  The world kernels take the env id as a launch argument, so a re-based pool needs its
    chunk graph captured again: one capture per ``rollout(net)``.

    The private Runner neither stashes activations nor bootstraps (the scan reads the last step's rows as the env left
    them), and plays through a "roll" workspace of its own: what a training rollout left in the net for its update, and the
    buffers its captured graphs point at, are as they were.  ``uniform_fn(t, E, 0)`` sees the GLOBAL step index t, and so does
    ``normal_fn(t, E, 0)``: the N(0,1) noise of a continuous net on a pool with ``float_actions`` (``point.DevicePointPool``),
    whose actions are float rows of ``pool.n_act``."""

    ENV_ID0 = 10007

    def __init__(self, hyps, pool, uniform_fn=None, keep_actions=False, normal_fn=None, norm=None):
        # norm: the training Runner's DeviceVecNorm (or a callable that returns it) under hyps norm_obs: the private Runner
        # normalises its observations by that block in frozen mode and never writes it; rewards stay the game's
        self.norm = norm
        if bool(try_key(hyps, "norm_obs", False)) and norm is None:
            raise ValueError("norm_obs: DeviceStatsRunner normalises by the training Runner's block: pass norm=runner.vecnorm")
        if not hasattr(pool, "device_step_post"):
            raise ValueError(f"DeviceStatsRunner: a device env pool with device_step_post ({' / '.join(families.FAMILIES)} "
                             "worlds)")
        self.pool, self.uniform_fn, self.keep_actions = pool, uniform_fn, bool(keep_actions)
        self.normal_fn = normal_fn                # continuous nets on a float-action pool: (t, E, 0) -> (E, n) device N(0,1)
        self.float_pool = bool(getattr(pool, "float_actions", False))
        self.E = len(pool)
        self.K = int(try_key(hyps, "eval_chunk", None) or 32)
        self.max_steps = int(try_key(hyps, "max_eval_steps", None) or 10 ** 6)
        if self.K < 1 or self.max_steps < 1:
            raise ValueError("DeviceStatsRunner: eval_chunk >= 1 and max_eval_steps >= 1")
        self.hyps = dict(hyps, n_envs=self.E, n_rollouts=self.E, n_tsteps=self.K)
        self._norm_obs = bool(self.hyps.pop("norm_obs", False))
        self.hyps.pop("norm_rewards", None)
        self.hyps.pop("bootstrap_truncated", None)      # (a key of the training targets: an evaluation has none)
        self.calls, self.last = 0, None
        self.runner = self.datas = None
        self._chunk = 0

    def _uniforms(self, t, B, env0):
        return self.uniform_fn(self._chunk * self.K + t, B, env0)

    def _normals(self, t, B, env0):
        return self.normal_fn(self._chunk * self.K + t, B, env0)

    def _setup(self, net):
        E, K, dev = self.E, self.K, net._dev
        C = int(self.hyps["n_frame_stack"])
        n = E * K
        f32 = dict(dtype=torch.float32, device=dev)
        D = dict(states=torch.zeros((n, C) + tuple(self.pool.frame_shape[1:]), **f32), deltas=torch.zeros(n, **f32),
                 rewards=torch.zeros(n, **f32), dones=torch.zeros(n, **f32),
                 actions=torch.zeros((n, int(self.pool.n_act)), **f32) if self.float_pool else
                 torch.zeros(n, dtype=torch.int64, device=dev))
        if net.is_recurrent:
            D["h_states"] = torch.zeros((n, net.h_size), **f32)
        self.datas = D
        self.runner = Runner(D, self.hyps, None, None, None, env_pool=self.pool,
                             uniform_fn=None if self.uniform_fn is None else self._uniforms,
                             normal_fn=None if self.normal_fn is None else self._normals, stash=False, bootstrap=False,
                             frozen_norm=None if not self._norm_obs else (self.norm() if callable(self.norm) else self.norm))
        self.ep_rew = torch.zeros(E, **f32)
        self.ep_len, self.active = (torch.zeros(E, dtype=torch.int32, device=dev) for _ in range(2))
        self.n_active = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ones = torch.ones(E, **f32)
        self._ws = ops.Workspace(dev)

    def _restart(self, net):
        """fresh worlds for this call, and the Runner's carried state as ``pool.start(runner)`` leaves it"""
        pool, r = self.pool, self.runner
        if not r._ready:
            r.start(net)
        r._dev_graphs.clear()          # (graphs of the ids the pool leaves: never replayed again)
        pool.reset_all(env_id0=self.ENV_ID0 + self.calls * self.E)
        ops.frame_stack_push(pool.frames, self._ones, r.bookmark.data_ptr(), r.S, r.bookmark.data_ptr(), r.S, self.E, r.C, r.HW)
        if r.vecnorm is not None:
            r.vecnorm.launch(self.E, 0, out_ptr=r.bookmark.data_ptr(), out_stride=r.S, C=r.C, update=False)
        r.val_prev.zero_()
        r.done_eff.zero_()
        if r.h is not None:
            r.h.zero_()
        self.ep_rew.zero_()
        self.ep_len.zero_()
        self.active.fill_(1)

    def rollout(self, net):
        if not getattr(net, "is_discrete", True) and not self.float_pool:
            raise ValueError("DeviceStatsRunner: the device worlds take discrete actions; the net is continuous")
        net._ensure_device()
        if self.runner is None:
            self._setup(net)
        E, K, D = self.E, self.K, self.datas
        slots = list(range(E))
        kept = dict(actions=[], rewards=[], dones=[])
        # the evaluation's forwards run through a "roll" workspace of their own: the training rollout's buffers (its graphs
        # hold their addresses) neither move nor change
        roll = net._ws.get("roll")
        net._ws["roll"] = self._ws
        try:
            self._restart(net)
            chunk = 0
            while True:
                self._chunk = chunk
                self.runner.rollout(net, slots, self.hyps)
                ops.eval_scan(D["rewards"], D["dones"], K, K, E, chunk * K, self.max_steps, self.ep_rew, self.ep_len,
                              self.active, self.n_active)
                if self.keep_actions:
                    for k in kept:
                        kept[k].append(D[k].view(E, K, *D[k].shape[1:]).transpose(0, 1).clone())
                left = int(self.n_active.item())               # the one host read of the chunk
                chunk += 1
                if left == 0 or chunk * K >= self.max_steps:
                    break
        finally:
            if roll is None:
                net._ws.pop("roll", None)
            else:
                net._ws["roll"] = roll
        self.calls += 1
        steps = min(chunk * K, self.max_steps)
        ep_rew = self.ep_rew.cpu()
        self.last = dict(ep_rew=ep_rew, ep_len=self.ep_len.cpu(), active=self.active.cpu(), steps=steps, chunks=chunk)
        for k, v in kept.items():
            if self.keep_actions:
                self.last[k] = torch.cat(v)[:steps].cpu()
        return float(ep_rew.double().sum()) / E
