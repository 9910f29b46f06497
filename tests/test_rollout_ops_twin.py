"""CPU: a NumPy float32 twin of one env step of Runner.rollout (runner.py:199-245 of the reference) batched over B envs, in
the shape the per-step rollout kernels of csrc/rollout_ops.hip have it -- and the proof that the twin is that env step.

The twin is what tests/test_gpu_rollout_ops.py compares the kernels with, bit for bit.  It must not be its own only
witness, so here `oracle.a2c_oracle.SlotRunner` (the batch-1 port of the reference's loop) plays scripted envs with a stub
net, and the twin, fed the same rewards / dones / frames / values / hidden rows as plain arrays, has to reproduce
SlotRunner's `states`, `rewards`, `dones`, `deltas` and `h_states` with np.array_equal: C in {1, 4}, Pong override on and
off, recurrent and not, several slots of T steps, two consecutive rollouts, rewards on non-terminal steps.

The TD residual is stated as include/a2c_mi355x.h states it, ((r_prev + (g * v) * (1 - d_prev)) - v_prev), every
intermediate a float32 and gamma itself rounded to float32 first; NumPy's float32 ufuncs round every operation and never
contract.  The valid-plane counts of the single-frame store (which the reference does not have) are held to the states:
expanding the twin's store with the twin's counts has to give SlotRunner's states.
"""
import numpy as np
import pytest
import torch

from oracle import a2c_oracle as O
from cases import hashf

NV_CAP = 4          # a2c_rollout_post_frames: the valid-plane count saturates at 4 (the store is four planes deep)


def f32(x):
    return np.asarray(x, dtype=np.float32)


def rndf(shape, seed, lo=-1.0, hi=1.0):
    """seeded uniform float32 at full resolution (hashf has 256 distinct values: too few to exercise a rounding)"""
    return (np.random.default_rng(seed).random(shape) * (hi - lo) + lo).astype(np.float32)


def td_delta(r_prev, d_prev, gamma, v, v_prev):
    """((r_prev + (g * v) * (1 - d_prev)) - v_prev), float32 at every step"""
    g = np.float32(gamma)
    gv = f32(g * f32(v))
    live = f32(np.float32(1) - f32(d_prev))
    return f32(f32(f32(r_prev) + f32(gv * live)) - f32(v_prev))


def new_rollout(n_slots, T, C=0, HW=0, hdim=0, fill=None):
    """rollout-major buffers (element e = slot * T + t).  fill: {name: value} sentinels, default zeros"""
    fill = fill or {}
    N = n_slots * T
    D = {k: np.full((N,), fill.get(k, 0), np.float32) for k in ("rewards", "dones", "deltas")}
    D["nvalid"] = np.full((N,), fill.get("nvalid", 0), np.int32)
    if C:
        D["states"] = np.full((N, C, HW), fill.get("states", 0), np.float32)
    if hdim:
        D["h_states"] = np.full((N, hdim), fill.get("h_states", 0), np.float32)
    return D


def new_carry(B, C=0, HW=0, hdim=0, fill=None):
    """what one env carries from step to step and from slot to slot"""
    fill = fill or {}
    car = dict(val_prev=np.full((B,), fill.get("val_prev", 0), np.float32),
               done_eff=np.full((B,), fill.get("done_eff", 0), np.float32),
               nv=np.full((B,), fill.get("nv", 1), np.int32))
    if C:
        car["state"] = np.full((B, C, HW), fill.get("state", 0), np.float32)
    if hdim:
        car["h"] = np.full((B, hdim), fill.get("h", 0), np.float32)
    return car


def twin_begin(D, car, T, slot0):
    """start of a slot: row 0 of every covered slot is what the env carried over (runner.py:199,201 at i == 0)"""
    e0 = (slot0 + np.arange(len(car["val_prev"]))) * T
    if "states" in D:
        D["states"][e0] = car["state"]
    if "h_states" in D:
        D["h_states"][e0] = car["h"]
    D["nvalid"][e0] = car["nv"]


def twin_step(D, car, rew, done, val, frame, T, t, slot0, gamma, pong, h_new=None, reset=None):
    """env step t of B envs (runner.py:207-232): rewards / dones rows, the TD residual of the step before, the next state
    (rows t + 1, or the carry at the end of the slot), the hidden row of the next step and the valid-plane count of the
    next state.  `done`: any nonzero ends the episode; `reset` (default: done != 0) is the frame stack's mask;
    `h_new`: what the cell of this step left."""
    rew, done, val = f32(rew), f32(done), f32(val)
    B = rew.shape[0]
    e = (slot0 + np.arange(B)) * T + t
    ended = done != 0
    reset = ended if reset is None else (f32(reset) != 0)
    d_eff = ended | (bool(pong) & (rew != 0))                      # runner.py:213-214
    D["rewards"][e] = rew
    D["dones"][e] = d_eff.astype(np.float32)
    car["done_eff"][:] = d_eff
    if t > 0:
        D["deltas"][e - 1] = td_delta(D["rewards"][e - 1], D["dones"][e - 1], gamma, val, car["val_prev"])
    car["val_prev"][:] = val
    if "states" in D:
        prev = D["states"][e]
        C = prev.shape[1]
        new = np.zeros_like(prev)
        new[:, :C - 1] = np.where(reset[:, None, None], np.float32(0), prev[:, 1:])      # utils.py:26-43
        new[:, C - 1] = f32(frame)
        if t + 1 < T:
            D["states"][e + 1] = new
        else:
            car["state"][:] = new
    nv = np.where(ended, 1, np.minimum(car["nv"] + 1, NV_CAP)).astype(np.int32)
    car["nv"][:] = nv
    if t + 1 < T:
        D["nvalid"][e + 1] = nv
    if h_new is not None:
        h = np.where(d_eff[:, None], np.float32(0), f32(h_new))   # runner.py:219-221
        car["h"][:] = h
        if t + 1 < T:
            D["h_states"][e + 1] = h


def twin_bootstrap(D, car, val_boot, T, slot0, gamma):
    """end of a slot (runner.py:236-245)"""
    val_boot = f32(val_boot)
    e = (slot0 + np.arange(val_boot.shape[0])) * T + T - 1
    r = D["rewards"][e].copy()
    open_ = D["dones"][e] == 0
    r[open_] = f32(r + f32(np.float32(gamma) * val_boot))[open_]
    D["rewards"][e] = r
    D["dones"][e] = np.where(open_, np.float32(1), D["dones"][e])
    D["deltas"][e] = f32(r - car["val_prev"])


def twin_store_begin(F, T, C):
    """single-frame store (R, T + C, HW) uint8: the frames the previous slot ended with move to the head of the window"""
    F[:, :C] = F[:, T:T + C].copy()


def twin_frames_to_states(F, nvalid, nt, C):
    """states (R, nt, C, HW) float32 out of the store: state k = frames k .. k + C - 1, planes c < C - nvalid[r, k] zero;
    nvalid (R, nt) or None (all valid)"""
    R, HW = F.shape[0], F.shape[2]
    out = np.zeros((R, nt, C, HW), np.float32)
    for k in range(nt):
        for c in range(C):
            live = np.ones(R, bool) if nvalid is None else (c >= C - nvalid[:, k])
            out[:, k, c] = np.where(live[:, None], F[:, k + c].astype(np.float32), np.float32(0))
    return out


# ============================================================================================ the twin held to SlotRunner
class ScriptEnv:
    """frames, rewards and dones out of arrays; reset() hands out the next reset frame"""

    def __init__(self, frames, rews, dones, reset_frames):
        self.frames, self.rews, self.dones, self.reset_frames = frames, rews, dones, reset_frames
        self.k = self.n_resets = 0

    def reset(self):
        f = self.reset_frames[self.n_resets]
        self.n_resets += 1
        return f[None].astype(np.float64)

    def step(self, action):
        k = self.k
        self.k += 1
        return self.frames[k][None].astype(np.float64), float(self.rews[k]), bool(self.dones[k]), {}


class StubNet:
    """scripted values, logits and hidden rows: call k of the net returns vals[k] (and h_rows[k])"""

    def __init__(self, vals, h_rows=None, n_actions=3):
        self.vals, self.h_rows, self.A = vals, h_rows, n_actions
        self.is_recurrent = h_rows is not None
        self.h_size = 0 if h_rows is None else h_rows.shape[1]
        self.k = 0

    def __call__(self, x, h=None):
        k = self.k
        self.k += 1
        val = torch.tensor([[self.vals[k]]], dtype=torch.float32)
        logits = torch.from_numpy(hashf(self.A, 900 + k, -1, 1))[None]
        if self.is_recurrent:
            assert h is not None and h.shape == (1, self.h_size)
            return val, logits, torch.from_numpy(self.h_rows[k].copy())[None]
        return val, logits


def _script(B, n_steps, HW, seed, hdim):
    """per env: frames (uint8 values), rewards nonzero on about half of the steps (terminal or not), dones on about a
    fifth, values, hidden rows; two net calls per step are budgeted (the bootstrap takes one more per slot)"""
    S = {}
    S["frames"] = np.floor(hashf(B * n_steps * HW, seed, 0, 256)).clip(0, 255).reshape(B, n_steps, HW).astype(np.float32)
    S["resets"] = np.floor(hashf(B * (n_steps + 2) * HW, seed + 1, 0, 256)).clip(0, 255).reshape(B, n_steps + 2, HW).astype(np.float32)
    r = rndf((B, n_steps), seed + 2, -2, 2)
    r[hashf(B * n_steps, seed + 3, 0, 1).reshape(B, n_steps) < 0.5] = 0
    S["rews"] = r
    S["dones"] = hashf(B * n_steps, seed + 4, 0, 1).reshape(B, n_steps) < 0.2
    S["vals"] = rndf((B, 2 * n_steps), seed + 5, -3, 3)
    S["h"] = rndf((B, 2 * n_steps, max(hdim, 1)), seed + 6, -1, 1)
    return S


@pytest.mark.parametrize("rec", [False, True])
@pytest.mark.parametrize("pong", [False, True])
@pytest.mark.parametrize("C", [1, 4])
def test_twin_reproduces_slot_runner_bit_for_bit(C, pong, rec):
    B, T, slot0, n_slots, HW, hdim, gamma, n_roll = 6, 5, 2, 10, 8, (3 if rec else 0), 0.99, 2
    hyps = dict(n_tsteps=T, gamma=gamma, n_frame_stack=C, action_shift=0, env_type="Pong-v0" if pong else "Breakout-v0")
    S = _script(B, n_roll * T, HW, 7 + C, hdim)
    N = n_slots * T
    Do = dict(states=torch.zeros(N, C, HW), rewards=torch.zeros(N), dones=torch.zeros(N), deltas=torch.zeros(N),
              actions=torch.zeros(N).long())
    if rec:
        Do["h_states"] = torch.zeros(N, hdim)
    envs = [ScriptEnv(S["frames"][b], S["rews"][b], S["dones"][b], S["resets"][b]) for b in range(B)]
    nets = [StubNet(S["vals"][b], S["h"][b] if rec else None) for b in range(B)]
    runners = [O.SlotRunner(envs[b], Do, hyps, uniform_fn=lambda: 0.5) for b in range(B)]
    for b in range(B):
        runners[b].start(nets[b])

    D = new_rollout(n_slots, T, C, HW, hdim)
    car = new_carry(B, C, HW, hdim)
    car["state"][:, C - 1] = S["resets"][:, 1]          # reset 0 is SlotRunner.__init__'s, reset 1 start()'s
    n_resets = np.full(B, 2)
    F = np.zeros((B, T + C, HW), np.uint8)              # the single-frame store of the same rollouts
    F[:, T + C - 1] = S["resets"][:, 1]
    calls = np.zeros(B, int)                            # net calls so far, per env
    saw_plain_reward = saw_done = saw_boot = False
    for r in range(n_roll):
        for b in range(B):
            runners[b].rollout(nets[b], slot0 + b)
        twin_begin(D, car, T, slot0)
        twin_store_begin(F, T, C)
        for t in range(T):
            k = r * T + t
            done = S["dones"][:, k]
            frame = S["frames"][:, k].copy()
            for b in np.nonzero(done)[0]:               # utils.py:36: the step's frame is dropped for env.reset()'s
                frame[b] = S["resets"][b, n_resets[b]]
                n_resets[b] += 1
            idx = (np.arange(B), calls)
            twin_step(D, car, S["rews"][:, k], done.astype(np.float32), S["vals"][idx], frame, T, t, slot0, gamma, pong,
                      h_new=S["h"][idx][:, :hdim] if rec else None)
            F[:, t + C] = frame
            calls += 1
            saw_plain_reward |= bool(((S["rews"][:, k] != 0) & ~done).any())
            saw_done |= bool(done.any())
        boot = D["dones"][(slot0 + np.arange(B)) * T + T - 1] == 0
        saw_boot |= bool(boot.any()) and not bool(boot.all())
        twin_bootstrap(D, car, S["vals"][(np.arange(B), calls)], T, slot0, gamma)
        calls += boot                                   # SlotRunner asks the net only where the slot did not end
        for k_ in ("states", "rewards", "dones", "deltas") + (("h_states",) if rec else ()):
            assert np.array_equal(Do[k_].numpy(), D[k_]), (k_, r)
        assert [n.k for n in nets] == list(calls)
        if C == NV_CAP:                                 # the store and the valid-plane counts stand for the same states
            rows = (slot0 + np.arange(B))[:, None] * T + np.arange(T)
            st = twin_frames_to_states(F, D["nvalid"][rows], T, C)
            assert np.array_equal(st, D["states"][rows])
    assert saw_plain_reward and saw_done and saw_boot
    untouched = np.ones(N, bool)
    untouched[slot0 * T:(slot0 + B) * T] = False
    for k_ in ("rewards", "dones", "deltas"):
        assert not D[k_][untouched].any() and not Do[k_].numpy()[untouched].any()


def test_td_delta_is_the_header_chain_in_float32():
    """against the same chain in float64 rounded once per operation by hand"""
    n = 4096
    r, d = rndf(n, 1, -2, 2), (hashf(n, 2, 0, 1) < 0.3).astype(np.float32)
    v, vp = rndf(n, 3, -3, 3), rndf(n, 4, -3, 3)
    g = np.float32(0.99)
    want = np.empty(n, np.float32)
    for i in range(n):
        gv = np.float32(float(g) * float(v[i]))                      # the product of two floats is exact in double
        term = np.float32(float(gv) * float(np.float32(1.0 - float(d[i]))))
        want[i] = np.float32(float(np.float32(float(r[i]) + float(term))) - float(vp[i]))
    assert np.array_equal(td_delta(r, d, 0.99, v, vp), want)


def test_frame_store_is_refused_for_any_frame_stack_but_four():
    """Runner._frame_store: the store is four planes deep and a2c_rollout_post_frames saturates its counts at 4, so an
    eight-plane net keeps the fp32 states (needs no device: the refusal comes before any allocation)"""
    from types import SimpleNamespace

    from a2c_amd.runner import Runner
    pool = SimpleNamespace(seq_env=np.zeros(3, int), seq_start=np.zeros(3, int))
    for C, want in ((1, False), (2, False), (8, False), (4, True)):
        stub = SimpleNamespace(hyps={"frame_store": True}, HW=16, C=C, B=3, _fstore_ok=True, _fstore=None, env_pool=pool,
                               d_frames=torch.arange(3 * 16, dtype=torch.uint8).reshape(3, 16))
        fs = Runner._frame_store(stub, 5, 3, "cpu")
        assert (fs is not None) == want, C
        if want:
            assert fs[0].shape == (3, 5 + 4, 16) and torch.equal(fs[0][:, 5 + 3], stub.d_frames)
