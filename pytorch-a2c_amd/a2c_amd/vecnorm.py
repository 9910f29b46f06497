"""Running observation / reward normalisation of the vector worlds: what baselines' VecNormalize does
between the envs and the agent.

``RunningNorm`` is the host twin of csrc/vecnorm.hip in NumPy float64: the same operations in the same order, the 256-lane
partial sums and the halving tree included, so that the device block and the twin agree bit for bit.  ``DeviceVecNorm`` is the
block in device memory that a2c_vecnorm_step advances; the Runner launches it behind every step's post launch.

The rule, for a batch of B values x with running (count, mean, var):
    bm = sum x / B;  bv = sum (x - bm)^2 / B              (two passes)
    delta = bm - mean;  tot = count + B
    mean += delta * B / tot
    var = (var * count + bv * B + delta * delta * count * B / tot) / tot
    count = tot
Observations: fold the batch in, then fp32(clip((x - mean) / sqrt(var + eps), +-clip_obs)) by the updated moments.  Rewards:
ret = ret * gamma + r per env, fold the B values of ret in, fp32(clip(r / sqrt(var + eps), +-clip_rew)), then ret = 0 where
done.  Frozen (``update=False``): observations by the moments as they stand, nothing written, no reward part.
"""
import numpy as np

from .families import VECTOR_DEVICE_TYPES

LANES = 256
MAX_L = 64
COUNT0 = 1e-4
_KEYS = ("obs_count", "obs_mean", "obs_var", "ret_count", "ret_mean", "ret_var", "ret")
_CONF = ("L", "B_pool", "gamma", "eps", "clip_obs", "clip_rew")


def lane_sum(v):
    """sum over axis 0 of a float64 (B, ...) array in the kernel's order: lane i of 256 adds rows i, i + 256, ... in order, then
    a halving tree over the lanes (strides 128 .. 1)"""
    v = np.asarray(v, dtype=np.float64)
    part = np.zeros((LANES,) + v.shape[1:], dtype=np.float64)
    for k in range(0, v.shape[0], LANES):
        chunk = v[k:k + LANES]
        part[:chunk.shape[0]] = part[:chunk.shape[0]] + chunk
    stride = LANES // 2
    while stride > 0:
        part[:stride] = part[:stride] + part[stride:2 * stride]
        stride //= 2
    return part[0]


def fold(mean, var, count, x):
    """the moment-combination rule for the batch x (B, ...) -> (mean, var, count); every operation left to right"""
    n = np.float64(x.shape[0])
    bm = lane_sum(x) / n
    d = x - bm
    bv = lane_sum(d * d) / n
    delta = bm - mean
    tot = count + n
    m2 = var * count + bv * n + delta * delta * count * n / tot
    return mean + delta * n / tot, m2 / tot, tot


def _clip(v, c):
    return np.where(v < -c, -c, np.where(v > c, c, v))


def _check_shape(L, B_pool):
    if not 1 <= int(L) <= MAX_L or int(B_pool) < 1:
        raise ValueError(f"vecnorm: 1 <= L <= {MAX_L} and B_pool >= 1, got L={L}, B_pool={B_pool}")


def norm_settings(hyps):
    """what ``hyps`` asks of the normaliser: None without ``norm_obs`` / ``norm_rewards``, else dict(obs, rewards, clip_obs,
    clip_rew, eps); a ValueError names the key that is out of range"""
    obs, rew = bool(hyps.get("norm_obs", False)), bool(hyps.get("norm_rewards", False))
    if not obs and not rew:
        return None
    out = dict(obs=obs, rewards=rew)
    for key, name, dflt in (("norm_clip_obs", "clip_obs", 10.0), ("norm_clip_rew", "clip_rew", 10.0), ("norm_eps", "eps", 1e-8)):
        v = hyps.get(key, None)
        v = dflt if v is None else float(v)
        if not v > 0:
            raise ValueError(f"{key}: must be positive, got {v}")
        out[name] = v
    return out


def norm_key(hyps):
    """the key an error names: the first of norm_obs / norm_rewards that is set"""
    return "norm_obs" if hyps.get("norm_obs", False) else "norm_rewards"


def _ranks():
    """the ranks of this process's initialised process group, 1 without one.  The Runner is not handed the ``Shard`` of a
    sharded run, so a group above one rank is TAKEN for one: a caller that knows better passes ``Runner(ranks=...)``.  The
    WORLD_SIZE variable alone says nothing (a launcher may set it for runs that do not shard) and is not read"""
    try:
        import torch.distributed as dist
    except ImportError:
        return 1
    return int(dist.get_world_size()) if dist.is_available() and dist.is_initialized() else 1


def check_runner(hyps, pool, net, stepper, ranks=None):
    """what the Runner refuses under ``norm_obs`` / ``norm_rewards`` (a ValueError naming the key): host env pools, pixel
    frames or vectors above 64 floats, nets on the one-launch step kernel (``stepper``), a sharded run above one rank
    (``ranks``: the caller's ``Shard.world``; None: ``_ranks()``)"""
    if norm_settings(hyps) is None:
        return
    key = norm_key(hyps)
    if (_ranks() if ranks is None else int(ranks)) > 1:
        raise ValueError(f"{key}: every rank of a sharded run would keep moments of its own envs and they would drift apart; "
                         "running normalisation is for one rank")
    if not hasattr(pool, "device_step_post"):
        raise ValueError(f"{key}: running normalisation lives in the slot of a DEVICE env pool "
                         f"({', '.join(VECTOR_DEVICE_TYPES)}); this is a host env pool")
    shape = tuple(pool.frame_shape)
    if len(shape) != 2 or shape[0] != 1 or not 1 <= shape[1] <= MAX_L:
        raise ValueError(f"{key}: running normalisation covers the vector worlds, frame_shape (1, L) with L <= {MAX_L}; this "
                         f"pool's frames are {shape}")
    if stepper:
        raise ValueError(f"{key}: a net on the one-launch step kernel stacks its frames inside that launch; FCModel / "
                         "GRUFCModel only")


class RunningNorm:
    """host twin of the device block: NumPy float64, bit-identical to a2c_vecnorm_step"""

    def __init__(self, L, B_pool, gamma, eps=1e-8, clip_obs=10, clip_rew=10):
        _check_shape(L, B_pool)
        if not eps > 0 or not clip_obs > 0 or not clip_rew > 0:
            raise ValueError("vecnorm: eps, clip_obs and clip_rew must be positive")
        self.L, self.B_pool = int(L), int(B_pool)
        self.gamma, self.eps = float(gamma), float(eps)
        self.clip_obs, self.clip_rew = float(clip_obs), float(clip_rew)
        self.obs_count, self.ret_count = np.float64(COUNT0), np.float64(COUNT0)
        self.obs_mean, self.obs_var = np.zeros(self.L), np.ones(self.L)
        self.ret_mean, self.ret_var = np.float64(0.0), np.float64(1.0)
        self.ret = np.zeros(self.B_pool)

    def normalize_obs(self, obs):
        """fp32(clip((x - mean) / sqrt(var + eps))) of (.., L) observations by the moments as they stand"""
        x = np.asarray(obs, dtype=np.float32).astype(np.float64)
        return _clip((x - self.obs_mean) / np.sqrt(self.obs_var + self.eps), self.clip_obs).astype(np.float32)

    def step(self, obs, rewards, dones, env0, update=True):
        """one env step of envs env0 .. env0+B-1: ``obs`` (B, L) or None, ``rewards`` / ``dones`` (B,) or None ->
        (normalised obs, normalised rewards) as float32 (None where absent)"""
        if obs is None and rewards is None:
            raise ValueError("vecnorm: both parts absent")
        if not update and rewards is not None:
            raise ValueError("vecnorm: the frozen mode normalises observations only")
        out_o = out_r = None
        if obs is not None:
            x = np.asarray(obs, dtype=np.float32).astype(np.float64).reshape(-1, self.L)
            self._range(env0, x.shape[0])
            if update:
                self.obs_mean, self.obs_var, self.obs_count = fold(self.obs_mean, self.obs_var, self.obs_count, x)
            out_o = self.normalize_obs(x)
        if rewards is not None:
            r = np.asarray(rewards, dtype=np.float32).astype(np.float64).reshape(-1)
            d = np.asarray(dones).reshape(-1)
            B = r.shape[0]
            self._range(env0, B)
            if d.shape[0] != B:
                raise ValueError("vecnorm: rewards and dones differ in length")
            sl = slice(env0, env0 + B)
            self.ret[sl] = self.ret[sl] * self.gamma + r
            self.ret_mean, self.ret_var, self.ret_count = fold(self.ret_mean, self.ret_var, self.ret_count, self.ret[sl])
            out_r = _clip(r / np.sqrt(self.ret_var + self.eps), self.clip_rew).astype(np.float32)
            self.ret[sl] = np.where(d != 0, 0.0, self.ret[sl])      # after the division, as baselines does
        return out_o, out_r

    def _range(self, env0, B):
        if B < 1 or env0 < 0 or env0 + B > self.B_pool:
            raise ValueError("vecnorm: env range outside the pool")

    # -- the block as a2c_vecnorm_step lays it out: 4 + 2 L + B_pool doubles
    def to_block(self):
        return np.concatenate([[self.obs_count], self.obs_mean, self.obs_var, [self.ret_count, self.ret_mean, self.ret_var],
                               self.ret]).astype(np.float64)

    def from_block(self, blk):
        blk = np.asarray(blk, dtype=np.float64).reshape(-1)
        L = self.L
        if blk.shape[0] != 4 + 2 * L + self.B_pool:
            raise ValueError("vecnorm: a block of another shape")
        self.obs_count, self.obs_mean, self.obs_var = blk[0].copy(), blk[1:1 + L].copy(), blk[1 + L:1 + 2 * L].copy()
        self.ret_count, self.ret_mean, self.ret_var = blk[1 + 2 * L].copy(), blk[2 + 2 * L].copy(), blk[3 + 2 * L].copy()
        self.ret = blk[4 + 2 * L:].copy()
        return self

    def state_dict(self):
        sd = {k: getattr(self, k) for k in _CONF}
        sd.update({k: np.array(getattr(self, k), dtype=np.float64) for k in _KEYS})
        return sd

    def load_state_dict(self, sd):
        if int(sd["L"]) != self.L or int(sd["B_pool"]) != self.B_pool:
            raise ValueError(f"vecnorm: the state is of L={sd['L']}, B_pool={sd['B_pool']}; this one of L={self.L}, "
                             f"B_pool={self.B_pool}")
        self.gamma, self.eps = float(sd["gamma"]), float(sd["eps"])
        self.clip_obs, self.clip_rew = float(sd["clip_obs"]), float(sd["clip_rew"])
        # (arrays, or the torch tensors a checkpoint holds them as)
        host = lambda v: np.array(v.numpy() if hasattr(v, "numpy") else v, dtype=np.float64)
        for k in ("obs_count", "ret_count", "ret_mean", "ret_var"):
            setattr(self, k, np.float64(host(sd[k]).reshape(())))
        for k, n in (("obs_mean", self.L), ("obs_var", self.L), ("ret", self.B_pool)):
            setattr(self, k, host(sd[k]).reshape(n))
        return self


class DeviceVecNorm:
    """the state block in device memory, advanced by a2c_vecnorm_step (one workgroup per launch; csrc/vecnorm.hip).  ``step``
    has the twin's surface on device tensors, in place; ``launch`` is what the Runner enqueues behind a step's post launch;
    ``snapshot`` / ``load`` move the block from / to a ``RunningNorm`` with one device read / write each"""

    def __init__(self, L, B_pool, gamma, eps=1e-8, clip_obs=10, clip_rew=10, device="cuda"):
        import torch
        from . import ops
        self._host = RunningNorm(L, B_pool, gamma, eps, clip_obs, clip_rew)      # (checks the arguments; keeps the settings)
        self.L, self.B_pool = self._host.L, self._host.B_pool
        self.block = torch.zeros(ops.vecnorm_state_doubles(self.L, self.B_pool), dtype=torch.float64, device=device)
        ops.vecnorm_init(self.block, self.L, self.B_pool)

    gamma = property(lambda self: self._host.gamma)
    eps = property(lambda self: self._host.eps)
    clip_obs = property(lambda self: self._host.clip_obs)
    clip_rew = property(lambda self: self._host.clip_rew)

    def launch(self, B, env0, out_ptr=0, out_stride=0, C=1, rewards=None, dones=None, T=1, t=0, slot0=0, update=True, st=None):
        """one a2c_vecnorm_step: the new plane of the B next-state rows at ``out_ptr`` (0: none) and / or row t of the slots'
        ``rewards`` (None: none).  Only enqueues: safe to capture"""
        from . import ops
        h = self._host
        if not update and rewards is None and out_ptr and B > 0:
            # frozen: no accumulator is touched, so the envs need not be the block's own (an evaluation pool of another size):
            # pieces of at most B_pool rows, each as envs 0 ..
            for k in range(0, B, self.B_pool):
                n = min(self.B_pool, B - k)
                ops.vecnorm_step(self.block, ops.vecnorm_args(n, 0, self.B_pool, self.L, C=C, update=False,
                                                              out_ptr=out_ptr + 4 * out_stride * k, out_stride=out_stride,
                                                              gamma=h.gamma, eps=h.eps, clip_obs=h.clip_obs,
                                                              clip_rew=h.clip_rew), st=st)
            return
        ops.vecnorm_step(self.block, ops.vecnorm_args(B, env0, self.B_pool, self.L, C=C, update=update, out_ptr=out_ptr,
                                                      out_stride=out_stride, rewards=rewards, dones=dones, T=T, t=t,
                                                      slot0=slot0, gamma=h.gamma, eps=h.eps, clip_obs=h.clip_obs,
                                                      clip_rew=h.clip_rew), st=st)

    def step(self, obs, rewards, dones, env0, update=True):
        """the twin's ``step`` on device tensors, IN PLACE: ``obs`` (B, L) float32 contiguous or None, ``rewards`` / ``dones``
        (B,) float32 or None -> (obs, rewards)"""
        from . import ops
        if obs is not None:
            ops._chk(obs, "obs")
            if obs.dim() != 2 or obs.shape[1] != self.L:
                raise ValueError(f"vecnorm: obs must be (B, {self.L})")
        B = obs.shape[0] if obs is not None else (rewards.shape[0] if rewards is not None else 0)
        self.launch(B, env0, out_ptr=0 if obs is None else obs.data_ptr(), out_stride=self.L, C=1, rewards=rewards,
                    dones=dones, T=1, t=0, slot0=0, update=update)
        return obs, rewards

    def snapshot(self):
        """-> a ``RunningNorm`` holding the block as it stands (one device read)"""
        h = self._host
        return RunningNorm(self.L, self.B_pool, h.gamma, h.eps, h.clip_obs, h.clip_rew).from_block(self.block.cpu().numpy())

    def load(self, norm):
        """the block := a ``RunningNorm`` (or its ``state_dict``); its settings come along (one device write)"""
        import torch
        if isinstance(norm, dict):
            norm = RunningNorm(self.L, self.B_pool, self.gamma).load_state_dict(norm)
        if norm.L != self.L or norm.B_pool != self.B_pool:
            raise ValueError(f"vecnorm: the state is of L={norm.L}, B_pool={norm.B_pool}; this block of L={self.L}, "
                             f"B_pool={self.B_pool}")
        self._host = RunningNorm(self.L, self.B_pool, norm.gamma, norm.eps, norm.clip_obs, norm.clip_rew)
        self.block.copy_(torch.from_numpy(norm.to_block()))
        return self

    def state_dict(self):
        return self.snapshot().state_dict()

    def load_state_dict(self, sd):
        return self.load(sd)
