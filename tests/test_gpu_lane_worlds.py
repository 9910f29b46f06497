"""-m gpu: what the shared kernel of the one-lane-per-env worlds (csrc/lane_world.h: Point, CartPole, Pendulum) must get right
for every world at once, at the smallest shapes where it can go wrong.  B = 65 is two workgroups, the second with one live
lane; C = 1 has no older plane to move and C = 4 three; hidden rows of 200 floats make the ballot loop stride; the step cap
closes envs of both workgroups.  Every buffer a launch writes has a guard row past env B - 1 (the rollout rows a guard slot on
either side), and the rows of ``out`` / ``prev`` and of ``obs`` padding floats inside their stride, all pre-filled with a
sentinel.  After every step the one launch (post form) equals the plain step followed by a2c_rollout_post (no hidden rows) or
a2c_rollout_record + a2c_frame_stack_push (hidden rows) on a second pool with the same seed, ``torch.equal`` throughout, and
every sentinel is intact on both sides."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GAMMA = 0.99
B, T, SLOT0, HDIM, STEPS, PAD = 65, 3, 2, 200, 40, 4
ENV_ID0, SEED, CAP = 7, 5, 12
RULES = dict(frame_skip=2, frame_skip_max=4, sticky_num=1, sticky_den=4)
SENT = -7

# world -> the pool's module and class, floats of an observation, actions of an env (0: one int64), what else the world takes
WORLDS = {
    "point": ("DevicePointPool", 8, 2, dict(targets_to_win=2)),
    "cartpole": ("DeviceCartPolePool", 4, 0, {}),
    "pendulum": ("DevicePendulumPool", 4, 1, {}),
}


def _actions(world):
    """fixed seeded actions of STEPS steps: int64 of either sign (taken mod 2), or float rows wider than the quantiser's range"""
    n_act = WORLDS[world][2]
    g = torch.Generator().manual_seed(11)
    if n_act == 0:
        return torch.randint(-9, 10, (STEPS, B), generator=g).to(DEV), 1
    return (1.5 * torch.randn((STEPS, B, n_act), generator=g)).to(DEV), n_act


class _Side:
    """one pool on guarded memory and one set of guarded rollout buffers, rows addressed as in the Runner's buffers: slot0 + b,
    T rows per slot, S = C * HW + PAD floats a row"""

    def __init__(self, world, C, recurrent):
        from a2c_amd import ops
        cls, self.HW, _, kw = WORLDS[world]
        self.C, self.S = C, C * self.HW + PAD
        self.pool = p = getattr(importlib.import_module("a2c_amd." + world), cls)(B, DEV, seed=SEED, max_episode_steps=CAP,
                                                                                  env_id0=ENV_ID0, **RULES, **kw)
        f32 = dict(dtype=torch.float32, device=DEV)
        full = lambda *shape: torch.full(shape, float(SENT), **f32)
        # the pool's own tensors, each with a guard row past env B - 1
        self.state = torch.full((B + 1, p.words), SENT, dtype=torch.int32, device=DEV)
        self.frames, self.rew, self.done, self.reset = full(B + 1, self.HW), full(B + 1), full(B + 1), full(B + 1)
        p.state, p.frames, p.rew, p.done, p.reset_mask = self.state[:B], self.frames[:B], self.rew[:B], self.done[:B], self.reset[:B]
        p.reset_all()
        self.obs = full(B + 1, self.HW + PAD)                       # the post launch's observation rows: padded
        N = (SLOT0 + B + 1) * T                                     # SLOT0 guard slots in front, one behind
        self.states, self.bookmark = full(N, self.S), full(B + 1, self.S)
        self.rewards, self.dones, self.deltas = full(N), full(N), full(N)
        self.val_prev, self.done_eff = torch.cat([torch.zeros(B, **f32), full(1)]), full(B + 1)
        self.h = full(B + 1, HDIM) if recurrent else None
        ops.frame_stack_push(p.frames, torch.ones(B, **f32), self.bookmark.data_ptr(), self.S, self.bookmark.data_ptr(), self.S,
                             B, C, self.HW)

    def sp(self, t):
        return self.states.data_ptr() + 4 * (SLOT0 * T + t) * self.S

    def rows(self, t):
        return (self.sp(t + 1), T * self.S) if t + 1 < T else (self.bookmark.data_ptr(), self.S)

    def outputs(self):
        """everything a step writes, guards and padding included (the observation rows apart: the two sides lay them out
        differently)"""
        out = dict(state=self.state, rew=self.rew, done=self.done, reset=self.reset, ep_stats=self.pool.ep_stats,
                   rewards=self.rewards, dones=self.dones, deltas=self.deltas, val_prev=self.val_prev, states=self.states,
                   bookmark=self.bookmark)
        if self.h is not None:
            out.update(h=self.h, done_eff=self.done_eff)
        return out

    def sentinels(self):
        """the guard rows and the padding floats"""
        lo, hi, n = SLOT0 * T, (SLOT0 + B) * T, self.C * self.HW
        g = [self.state[B:], self.frames[B:], self.rew[B:], self.done[B:], self.reset[B:], self.obs[B:], self.obs[:, self.HW:],
             self.states[:lo], self.states[hi:], self.states[:, n:], self.bookmark[B:], self.bookmark[:, n:], self.val_prev[B:]]
        g += [x[i] for x in (self.rewards, self.dones, self.deltas) for i in (slice(0, lo), slice(hi, None))]
        if self.h is not None:
            g += [self.h[B:], self.done_eff[B:]]
        return g

    def intact(self):
        return all(bool((x == SENT).all()) for x in self.sentinels())


@pytest.mark.parametrize("recurrent", [False, True])
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("world", list(WORLDS))
def test_one_launch_equals_its_launch_sequence_inside_its_rows(world, C, recurrent):
    from a2c_amd import ops
    a, b = _Side(world, C, recurrent), _Side(world, C, recurrent)      # a: the launch sequence, b: one launch
    step_post = getattr(ops, world + "_step")
    acts, ld = _actions(world)
    g = torch.Generator().manual_seed(10 * C + recurrent)
    vals = torch.randn((STEPS, B, 2), generator=g).to(DEV)            # val_stride = 2
    hs = torch.randn((STEPS, B, HDIM), generator=g).to(DEV)
    HW, S, n = a.HW, a.S, C * a.HW
    assert a.intact() and b.intact() and torch.equal(a.frames, b.frames) and torch.equal(a.state, b.state)
    closed = torch.zeros(B, dtype=torch.bool, device=DEV)
    for k in range(STEPS):
        t = k % T
        if t == 0:       # state 0 of a slot = the bookmark
            for x in (a, b):
                x.states.view(-1, T, S)[SLOT0:SLOT0 + B, 0, :n] = x.bookmark[:B, :n]
        if recurrent:
            a.h[:B] = hs[k]
            b.h[:B] = hs[k]
        ap, v = acts[k].data_ptr(), vals[k]
        fr, rew, done, reset = a.pool.step(ap, ld)
        nxt, nstride = a.rows(t)
        if recurrent:
            ops.rollout_record(a.rew, a.done, v.data_ptr(), 2, a.val_prev, a.rewards, a.dones, a.deltas, a.done_eff, a.h, B, T, t,
                               SLOT0, GAMMA, False)
            ops.frame_stack_push(a.frames, a.reset, a.sp(t), T * S, nxt, nstride, B, C, HW)
        else:
            ops.rollout_post(a.rew, a.done, v.data_ptr(), 2, a.val_prev, a.rewards, a.dones, a.deltas, T, t, SLOT0, GAMMA, False,
                             a.frames, a.reset, a.sp(t), T * S, nxt, nstride, B, C, HW)
        nxt, nstride = b.rows(t)
        post = ops.world_post(v.data_ptr(), 2, b.val_prev, b.rewards, b.dones, b.deltas, T, t, SLOT0, GAMMA, False, b.sp(t), T * S,
                              nxt, nstride, C, done_eff=b.done_eff if recurrent else None, h=b.h)
        p = b.pool
        step_post(b.state, ap, ld, p.action_shift, B, p.env_id0, p.seed, *p.world, b.obs, HW + PAD, b.rew, b.done, b.reset,
                  p.rules, post, p.ep_stats[0:1], p.ep_stats[1:2])
        oa, ob = a.outputs(), b.outputs()
        for name in oa:
            assert torch.equal(oa[name], ob[name]), (world, C, k, name)
        assert torch.equal(b.obs[:B, :HW], fr), (world, C, k, "obs")
        assert a.intact() and b.intact(), (world, C, k, "a guard row or a padding float was written")
        if recurrent:
            rows = done.bool()
            assert bool((b.h[:B][rows] == 0).all()) and torch.equal(b.h[:B][~rows], hs[k][~rows])
        closed |= done.bool()
    assert bool(closed[:64].any()) and bool(closed[64]), "envs of both workgroups closed"
    assert int(a.pool.ep_stats[0]) >= B
