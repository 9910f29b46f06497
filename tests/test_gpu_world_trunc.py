"""-m gpu: time-limit truncation on the lane worlds (hyps bootstrap_truncated), from the kernel up.

  * a2c_<world>_step_trunc against the host twins and against a2c_<world>_step run from the same state, at the lane and
    wavefront edges, plain and with frame skip + sticky actions, without and with a post block, into strided rows whose gaps
    and guard rows hold a sentinel; the rejected argument blocks;
  * a2c_final_states against an index expression, a2c_trunc_bootstrap against its fp32 host statement;
  * the update: rollouts with the key on, then a second Updater with the key OFF, fed rewards / deltas doctored on the host by
    the fp32 statement from the first Updater's ``vfin``, must land on the same parameters and the same five scalars, bit for
    bit -- eager, captured, on the eager rollout loop, and under running normalisation;
  * the key off: no new buffers, and a run identical to one without the key.

The worlds are integers and every float operation has a stated order, so every comparison is bit equality."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cases import base_hyps  # noqa: E402
from test_world_trunc import CARTPOLE_CAP, PUSH  # noqa: E402

DEV = "cuda"
GAMMA = 0.99
SENT = -7.0
CAP, STEPS, T = 3, 12, 3
ENV_ID0, SEED = 7, 5
SIZES = (1, 63, 64, 65, 130)
REPEATS = {"plain": dict(), "skip2_sticky": dict(frame_skip=2, sticky_num=1, sticky_den=4)}

# world -> pool class, twin class, floats of an observation, floats of an action (0: one int64), what else the world takes
WORLDS = {
    "point": ("DevicePointPool", "PointEnv", 8, 2, dict(targets_to_win=1)),
    "cartpole": ("DeviceCartPolePool", "CartPoleEnv", 4, 0, {}),
    "pendulum": ("DevicePendulumPool", "PendulumEnv", 4, 1, {}),
}


def _bits(a, b, what):
    a, b = (np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x) for x in (a, b))
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)
    if bad.any():
        i = int(np.argwhere(bad)[0][0]) // a.dtype.itemsize
        print(f"{what}: first difference at flat {i}: {a.reshape(-1)[i]!r} vs {b.reshape(-1)[i]!r}")
    assert not bad.any(), what


def _actions(world, B):
    n_act = WORLDS[world][3]
    g = torch.Generator().manual_seed(11)
    if n_act == 0:
        return torch.randint(-9, 10, (STEPS, B), generator=g).to(DEV), 1
    return (1.5 * torch.randn((STEPS, B, n_act), generator=g)).to(DEV), n_act


class _Side:
    """one pool and, with C, the rollout rows of a post block (slot0 = 0, T rows per slot)"""

    def __init__(self, world, B, C, repeat):
        from a2c_amd import ops
        mod = importlib.import_module("a2c_amd." + world)
        cls, _, self.HW, _, kw = WORLDS[world]
        self.B, self.C = B, C
        self.pool = p = getattr(mod, cls)(B, DEV, seed=SEED, max_episode_steps=CAP, env_id0=ENV_ID0, **repeat, **kw)
        p.reset_all()
        f32 = dict(dtype=torch.float32, device=DEV)
        self.obs = torch.zeros((B, self.HW), **f32)
        if C:
            self.S = S = C * self.HW
            self.states, self.bookmark = torch.zeros((B * T, S), **f32), torch.zeros((B, S), **f32)
            self.rewards, self.dones, self.deltas = (torch.zeros(B * T, **f32) for _ in range(3))
            self.val_prev = torch.zeros(B, **f32)
            ops.frame_stack_push(p.frames, torch.ones(B, **f32), self.bookmark.data_ptr(), S, self.bookmark.data_ptr(), S, B, C,
                                 self.HW)

    def post(self, t, vals):
        from a2c_amd import ops
        if not self.C:
            return None
        S, B = self.S, self.B
        if t == 0:
            self.states.view(B, T, S)[:, 0] = self.bookmark
        sp = self.states.data_ptr() + 4 * t * S
        nxt, nstride = (sp + 4 * S, T * S) if t + 1 < T else (self.bookmark.data_ptr(), S)
        return ops.world_post(vals.data_ptr(), 1, self.val_prev, self.rewards, self.dones, self.deltas, T, t, 0, GAMMA, False, sp,
                              T * S, nxt, nstride, self.C)

    def outputs(self):
        p = self.pool
        out = dict(state=p.state, obs=self.obs, rew=p.rew, done=p.done, reset=p.reset_mask, ep_stats=p.ep_stats)
        if self.C:
            out.update(states=self.states, bookmark=self.bookmark, rewards=self.rewards, dones=self.dones, deltas=self.deltas,
                       val_prev=self.val_prev)
        return out


def _step(world, side, ap, ld, post, tr=False):
    """the plain step, or with ``tr`` (a ``world_trunc`` block; None: a NULL one) a2c_<world>_step_trunc"""
    from a2c_amd import ops
    p = side.pool
    head = (p.state, ap, ld, p.action_shift, side.B, p.env_id0, p.seed, *p.world, side.obs, side.HW, p.rew, p.done, p.reset_mask)
    tail = (p.rules, post, p.ep_stats[0:1], p.ep_stats[1:2])
    if tr is False:
        getattr(ops, world + "_step")(*head, *tail)
    else:
        getattr(ops, world + "_step_trunc")(*head, tr, *tail)


@pytest.mark.parametrize("C", [0, 1, 3], ids=["nopost", "C1", "C3"])
@pytest.mark.parametrize("repeat", list(REPEATS))
@pytest.mark.parametrize("world", list(WORLDS))
def test_step_trunc_equals_the_twin_and_the_plain_step(world, repeat, C):
    from a2c_amd import ops
    mod = importlib.import_module("a2c_amd." + world)
    _, twin_cls, HW, n_act, kw = WORLDS[world]
    seen_trunc = seen_term = 0
    for B in SIZES:
        a, b = _Side(world, B, C, REPEATS[repeat]), _Side(world, B, C, REPEATS[repeat])     # a: step_trunc, b: the plain step
        twins = [getattr(mod, twin_cls)(seed=SEED, env_id=ENV_ID0 + j, max_episode_steps=CAP, **REPEATS[repeat], **kw)
                 for j in range(B)]
        for e in twins:
            e.reset()
        acts, ld = _actions(world, B)
        host_acts = acts.cpu().numpy()
        g = torch.Generator().manual_seed(B)
        vals = torch.randn((STEPS, B), generator=g).to(DEV)
        # rows (b, t) of a buffer of B slots x T steps and one guard slot, as the Runner lays them out: strides T and T * HW
        truncs = torch.full(((B + 1) * T,), SENT, device=DEV)
        final = torch.full(((B + 1) * T, HW), SENT, device=DEV)
        want_tr, want_fin = truncs.cpu().numpy().copy(), final.cpu().numpy().copy()
        for k in range(STEPS):
            t = k % T
            ap = acts[k].data_ptr()
            tr = ops.world_trunc(truncs.data_ptr() + 4 * t, T, final.data_ptr() + 4 * t * HW, T * HW)
            _step(world, a, ap, ld, a.post(t, vals[k]), tr)
            _step(world, b, ap, ld, b.post(t, vals[k]))
            oa, ob = a.outputs(), b.outputs()
            for name in oa:
                _bits(oa[name], ob[name], (world, repeat, C, B, k, name))
            obs, rew, done = (np.zeros((B, HW), np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32))
            for j, e in enumerate(twins):
                act = host_acts[k, j] if n_act else int(host_acts[k, j])
                o, rew[j], d, _ = e.step(act)
                want_tr[j * T + t], want_fin[j * T + t] = float(e.truncated), e.final_obs.reshape(HW)
                seen_trunc += e.truncated
                seen_term += d and not e.truncated
                done[j] = float(d)
                obs[j] = np.asarray(e.reset() if d else o, dtype=np.float32).reshape(HW)
            what = (world, repeat, C, B, k)
            _bits(a.obs, obs, what + ("obs",))
            _bits(a.pool.rew, rew, what + ("rew",))
            _bits(a.pool.done, done, what + ("done",))
            _bits(a.pool.reset_mask, done, what + ("reset",))
            _bits(truncs, want_tr, what + ("trunc, its gaps and its guard slot",))
            _bits(final, want_fin, what + ("final_obs, its gaps and its guard slot",))
            if C:
                _bits(a.bookmark.view(B, C, HW)[:, C - 1] if t == T - 1 else a.states.view(B, T, C, HW)[:, t + 1, C - 1], obs,
                      what + ("the new plane",))
    assert seen_trunc >= len(SIZES), "the step limit ended episodes"
    if world == "pendulum":
        assert seen_term == 0, "only the limit ends a Pendulum episode"


def test_cartpole_kernel_sees_both_kinds_of_close():
    """the inputs of tests/test_world_trunc.py: envs 0-2 push one way and fall (terminal), envs 3-4 alternate and reach the cap"""
    from a2c_amd import cartpole, ops
    B, n = 5, 40
    pool = cartpole.DeviceCartPolePool(B, DEV, seed=5, max_episode_steps=CARTPOLE_CAP)
    pool.reset_all()
    twins = [cartpole.CartPoleEnv(seed=5, env_id=j, max_episode_steps=CARTPOLE_CAP) for j in range(B)]
    for e in twins:
        e.reset()
    truncs, final = torch.full((B,), SENT, device=DEV), torch.full((B, 4), SENT, device=DEV)
    obs = torch.zeros((B, 4), device=DEV)
    kinds = set()
    for k in range(n):
        act = torch.tensor([PUSH["constant" if j < 3 else "alternating"](k) for j in range(B)], dtype=torch.int64, device=DEV)
        ops.cartpole_step_trunc(pool.state, act.data_ptr(), 1, 0, B, 0, pool.seed, CARTPOLE_CAP, obs, 4, pool.rew, pool.done,
                                pool.reset_mask, ops.world_trunc(truncs.data_ptr(), 1, final.data_ptr(), 4))
        want_t, want_f = np.zeros(B, np.float32), np.zeros((B, 4), np.float32)
        for j, e in enumerate(twins):
            _, _, d, _ = e.step(int(act[j]))
            want_t[j], want_f[j] = float(e.truncated), e.final_obs.reshape(4)
            if d:
                kinds.add("truncated" if e.truncated else "terminal")
                e.reset()
        _bits(truncs, want_t, (k, "trunc"))
        _bits(final, want_f, (k, "final_obs"))
    assert kinds == {"truncated", "terminal"}


@pytest.mark.parametrize("world", list(WORLDS))
def test_step_trunc_rejects_bad_blocks_and_writes_nothing(world):
    from a2c_amd import _lib, ops
    B = 5
    s = _Side(world, B, 0, {})
    HW = s.HW
    acts, ld = _actions(world, B)
    truncs, final = torch.full((B * T,), SENT, device=DEV), torch.full((B * T, HW + 4), SENT, device=DEV)
    before = {k: v.clone() for k, v in s.outputs().items()}
    tp, fp = truncs.data_ptr(), final.data_ptr()
    bad = [None, ops.world_trunc(0, T, fp, HW), ops.world_trunc(tp, T, 0, HW), ops.world_trunc(tp, 0, fp, HW),
           ops.world_trunc(tp, -1, fp, HW), ops.world_trunc(tp, T, fp, HW - 4), ops.world_trunc(tp, T, fp, HW + 2),
           ops.world_trunc(tp, T, fp + 4, HW), ops.world_trunc(tp, T, fp + 8, HW + 4)]
    for tr in bad:
        with pytest.raises(_lib.A2CKernelError, match="invalid argument"):
            _step(world, s, acts[0].data_ptr(), ld, None, tr)
    torch.cuda.synchronize()
    for k, v in s.outputs().items():
        _bits(v, before[k], (world, k))
    assert bool((truncs == SENT).all()) and bool((final == SENT).all())
    # and a good block, padded rows: only the HW floats of each row are written
    _step(world, s, acts[0].data_ptr(), ld, None, ops.world_trunc(tp, T, fp, T * (HW + 4)))
    assert bool((final.view(B, T, HW + 4)[:, 0, :HW] != SENT).all()) and bool((final.view(B, T, HW + 4)[:, 0, HW:] == SENT).all())
    assert bool((final.view(B, T, HW + 4)[:, 1:] == SENT).all()) and bool((truncs.view(B, T)[:, 1:] == SENT).all())
    assert bool((truncs.view(B, T)[:, 0] != SENT).all())


# ---------------------------------------------------------------- the two launchers of the update
@pytest.mark.parametrize("HW", [4, 8])
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("N", [1, 5, 260])
def test_final_states_equal_the_index_expression(N, C, HW):
    from a2c_amd import ops
    g = torch.Generator().manual_seed(N + 10 * C + HW)
    states = torch.randn((N, C, HW), generator=g).to(DEV)
    fin = torch.randn((N, HW), generator=g).to(DEV)
    out = torch.full((N + 1, C, HW), SENT, device=DEV)
    keep = states.clone(), fin.clone()
    ops.final_states(states, fin, C, HW, N, out[:N])
    want = torch.cat([states[:, 1:], fin[:, None]], dim=1)
    assert torch.equal(out[:N], want) and bool((out[N] == SENT).all())
    assert torch.equal(states, keep[0]) and torch.equal(fin, keep[1])


@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_trunc_bootstrap_equals_the_fp32_statement(N):
    from a2c_amd import ops
    rng = np.random.default_rng(N)
    mk = lambda s: (rng.standard_normal(N) * s).astype(np.float32)
    rew, dlt, vf = mk(3), mk(2), mk(5)
    tr = (rng.random(N) < 0.5).astype(np.float32)
    for x in (rew, dlt, vf):                    # zeros of either sign among a mix of signs
        x[rng.integers(0, N, size=max(1, N // 16))] = 0.0
        x[rng.integers(0, N, size=max(1, N // 16))] = -0.0
    tr[0] = 1.0
    d = lambda x: torch.from_numpy(x).to(DEV)
    for truncs in (tr, np.zeros(N, np.float32)):
        ro, do = torch.full((N + 1,), SENT, device=DEV), torch.full((N + 1,), SENT, device=DEV)
        ops.trunc_bootstrap(d(rew), d(dlt), d(truncs), d(vf), GAMMA, N, ro[:N], do[:N])
        _bits(ro[:N], ops.trunc_bootstrap_host(rew, truncs, vf, GAMMA), (N, "rewards"))
        _bits(do[:N], ops.trunc_bootstrap_host(dlt, truncs, vf, GAMMA), (N, "deltas"))
        assert float(ro[N]) == SENT and float(do[N]) == SENT
        if not truncs.any():
            _bits(ro[:N], rew, (N, "rewards pass through"))
            _bits(do[:N], dlt, (N, "deltas pass through"))
    # in place, as x_out may be x
    r2, d2 = d(rew), d(dlt)
    ops.trunc_bootstrap(r2, d2, d(tr), d(vf), GAMMA, N, r2, d2)
    _bits(r2, ops.trunc_bootstrap_host(rew, tr, vf, GAMMA), (N, "in place"))


# ---------------------------------------------------------------- rollout + update
B_ENVS, T_ROLL, C_ROLL = 5, 8, 2
N_ROLL = B_ENVS * T_ROLL
FAMILIES = {
    # family -> pool / twin module, L, action size, continuous, the cap
    "Pendulum": ("pendulum", 4, 1, True, CAP),
    "CartPole": ("cartpole", 4, 2, False, CARTPOLE_CAP),
}


def _net(L, n_act, cont, seed=5):
    import a2c_amd
    torch.manual_seed(seed)
    return a2c_amd.FCModel([C_ROLL, L], n_act, h_size=32, bnorm=False, is_discrete=not cont)


def _datas(L, n_act, cont, trunc):
    z = lambda *s: torch.zeros(*s, device=DEV)
    D = dict(states=z(N_ROLL, C_ROLL, L), deltas=z(N_ROLL), rewards=z(N_ROLL), dones=z(N_ROLL),
             actions=z(N_ROLL, n_act) if cont else torch.zeros(N_ROLL, dtype=torch.int64, device=DEV))
    if trunc:
        D.update(truncs=torch.full((N_ROLL,), SENT, device=DEV), final_obs=torch.full((N_ROLL, L), SENT, device=DEV))
    return D


def _setup(family, key=True, **kw):
    """-> (hyps, net, D, Runner, twins): the noise is fixed per (round, step), so two set-ups play the same game"""
    from a2c_amd.runner import Runner
    name, L, n_act, cont, cap = FAMILIES[family]
    mod = importlib.import_module("a2c_amd." + name)
    hyps = base_hyps(**dict(dict(env_type=family + "-device", n_tsteps=T_ROLL, n_rollouts=B_ENVS, n_envs=B_ENVS,
                                 n_frame_stack=C_ROLL, is_discrete=not cont, h_size=32, gamma=GAMMA, model="FCModel"), **kw))
    if key is not None:
        hyps["bootstrap_truncated"] = key
    net = _net(L, n_act, cont)
    D = _datas(L, n_act, cont, bool(key))
    pool = getattr(mod, f"Device{family}Pool")(B_ENVS, DEV, seed=5, max_episode_steps=cap)
    g = torch.Generator().manual_seed(4)
    eps, rnd = (1.5 * torch.randn((8, T_ROLL, B_ENVS, 1), generator=g)).to(DEV), [0]
    # CartPole: the sampler's uniforms pick the pushes of tests/test_world_trunc.py while the policy is near uniform: envs
    # 0-2 push right (u close to 1), envs 3-4 alternate
    u = torch.tensor([[0.999 if (j < 3 or (t % 2)) else 0.001 for j in range(B_ENVS)] for t in range(T_ROLL)], device=DEV)
    r = Runner(D, hyps, None, None, None, env_pool=pool,
               normal_fn=(lambda t, Bn, env0: eps[rnd[0], t, env0:env0 + Bn]) if cont else None,
               uniform_fn=None if cont else (lambda t, Bn, env0: u[t, env0:env0 + Bn]))
    twins = [getattr(mod, family + "Env")(seed=5, env_id=j, max_episode_steps=cap) for j in range(B_ENVS)]
    for e in twins:
        e.reset()
    return hyps, net, D, r, twins, rnd


def _replay_twins(twins, D, cont, L):
    """the recorded actions through the host twins -> (truncs (N,), final_obs (N, L), closes by kind) of this rollout"""
    acts = D["actions"].cpu().numpy().reshape(B_ENVS, T_ROLL, -1)
    tr, fin = np.zeros((B_ENVS, T_ROLL), np.float32), np.zeros((B_ENVS, T_ROLL, L), np.float32)
    kinds = dict(truncated=0, terminal=0)
    for t in range(T_ROLL):
        for j, e in enumerate(twins):
            _, _, d, _ = e.step(acts[j, t] if cont else int(acts[j, t, 0]))
            tr[j, t], fin[j, t] = float(e.truncated), e.final_obs.reshape(L)
            if d:
                kinds["truncated" if e.truncated else "terminal"] += 1
                e.reset()
    return tr.reshape(-1), fin.reshape(-1, L), kinds


def _update_rounds(family, rounds=3, capture=False, **kw):
    """rollout + update rounds with the key on, shadowed by an Updater with the key off on doctored buffers"""
    from a2c_amd import ops
    from a2c_amd.updater import Updater
    name, L, n_act, cont, cap = FAMILIES[family]
    hyps, net, D, r, twins, rnd = _setup(family, True, **kw)
    upd = Updater(net, hyps)
    upd.vecnorm = lambda: r.vecnorm
    off = {k: v for k, v in hyps.items() if k != "bootstrap_truncated"}
    net2 = _net(L, n_act, cont)
    net2.load_state_dict(net.state_dict())
    upd2 = Updater(net2, off)
    seen = dict(truncated=0, terminal=0)
    graph = None
    for rnd[0] in range(rounds):
        r.rollout(net, list(range(B_ENVS)), hyps)
        r.finish()
        # the rollout layer: rows (slot, t) of truncs / final_obs are the twins', every row written
        want_tr, want_fin, kinds = _replay_twins(twins, D, cont, L)
        _bits(D["truncs"], want_tr, (family, rnd[0], "truncs"))
        _bits(D["final_obs"], want_fin, (family, rnd[0], "final_obs"))
        for k in kinds:
            seen[k] += kinds[k]
        # the final states the critic must see, and its own forward on them at the same N, before the weights move
        last = torch.from_numpy(want_fin).to(DEV)
        if hyps.get("norm_obs"):
            last = torch.from_numpy(r.vecnorm.snapshot().normalize_obs(want_fin)).to(DEV)
        want_states = torch.cat([D["states"][:, 1:], last[:, None]], dim=1).contiguous()
        with torch.no_grad():
            want_v = net(want_states)[0].reshape(-1).clone()
        snap = {k: v.clone() for k, v in D.items()}
        if capture and rnd[0] >= 1:
            graph = graph or upd.capture_update(D)
            info = graph.replay()
        else:
            info = upd.update_model(D)
        for k in snap:
            assert torch.equal(D[k], snap[k]), (family, rnd[0], k, "shared_data must not be written by the update")
        b = upd._bufs
        _bits(b["fin"].view(N_ROLL, C_ROLL, L), want_states, (family, rnd[0], "final states"))
        _bits(b["vfin"], want_v, (family, rnd[0], "vfin against the net's own forward"))
        vfin = b["vfin"].cpu().numpy()
        trn = D["truncs"].cpu().numpy()
        D2 = dict(snap)
        D2.pop("truncs"), D2.pop("final_obs")
        for k in ("rewards", "deltas"):
            D2[k] = torch.from_numpy(ops.trunc_bootstrap_host(snap[k].cpu().numpy(), trn, vfin, GAMMA)).to(DEV)
        info2 = upd2.update_model(D2)
        assert list(info) == list(info2) and len(info) == 5
        for k in info:
            assert np.float64(info[k]).tobytes() == np.float64(info2[k]).tobytes(), (family, rnd[0], k, info[k], info2[k])
        for (n1, p1), (_, p2) in zip(net.named_parameters(), net2.named_parameters()):
            _bits(p1, p2, (family, rnd[0], n1))
        if kinds["truncated"]:
            assert not torch.equal(D2["rewards"], snap["rewards"]), "a truncated close changes the targets"
    return r, seen, graph


def test_pendulum_update_equals_the_key_off_update_on_doctored_buffers():
    r, seen, _ = _update_rounds("Pendulum")
    assert seen["truncated"] >= B_ENVS * 3 * T_ROLL // CAP - B_ENVS and seen["terminal"] == 0
    assert any(g not in ("warm", False) for g in r._dev_graphs.values()), "the slot was captured and replayed"


def test_cartpole_update_with_both_kinds_of_close_in_a_batch():
    r, seen, _ = _update_rounds("CartPole")
    assert seen["truncated"] >= 1 and seen["terminal"] >= 1, seen


def test_update_captured():
    _, seen, graph = _update_rounds("Pendulum", capture=True)
    assert graph is not None and len(graph.graphs) == 1 and graph.fallbacks == 0 and seen["truncated"] > 0


def test_update_on_the_eager_rollout_loop():
    r, seen, _ = _update_rounds("Pendulum", rollout_graphs=False)
    assert not r._dev_graphs and seen["truncated"] > 0


def test_update_under_running_normalisation():
    r, seen, _ = _update_rounds("Pendulum", norm_obs=True, norm_rewards=True)
    assert r.vecnorm is not None and seen["truncated"] > 0


def _plain_run(key):
    from a2c_amd.updater import Updater
    hyps, net, D, r, _, rnd = _setup("Pendulum", key)
    upd = Updater(net, hyps)
    rows = []
    for rnd[0] in range(2):
        r.rollout(net, list(range(B_ENVS)), hyps)
        r.finish()
        rows.append({k: v.clone() for k, v in D.items()})
        info = upd.update_model(D)
        rows.append({k: torch.tensor(v, dtype=torch.float64) for k, v in info.items()})
    assert "truncs" not in D and "final_obs" not in D and "vfin" not in upd._bufs
    return rows, [p.detach().clone() for p in net.parameters()], r.env_pool.state.clone()


def test_key_off_is_a_run_without_the_key():
    rows_a, params_a, state_a = _plain_run(None)
    rows_b, params_b, state_b = _plain_run(False)
    for ra, rb in zip(rows_a, rows_b):
        assert list(ra) == list(rb)
        for k in ra:
            assert torch.equal(ra[k], rb[k]), k
    for pa, pb in zip(params_a, params_b):
        assert torch.equal(pa, pb)
    assert torch.equal(state_a, state_b)


def test_runner_refuses_by_the_key():
    from a2c_amd import pendulum
    from a2c_amd.runner import Runner
    import a2c_amd
    hyps, net, D, r, _, _ = _setup("Pendulum", True)
    del D["truncs"]
    with pytest.raises(ValueError, match="bootstrap_truncated"):
        r.rollout(net, list(range(B_ENVS)), hyps)
    hyps, net, D, r, _, _ = _setup("Pendulum", True)
    torch.manual_seed(1)
    gru = a2c_amd.GRUFCModel([C_ROLL, 4], 1, h_size=32, bnorm=False, is_discrete=False)
    D["h_states"] = torch.zeros(N_ROLL, gru.h_size, device=DEV)
    r2 = Runner(D, hyps, None, None, None, env_pool=pendulum.DevicePendulumPool(B_ENVS, DEV, seed=5, max_episode_steps=CAP))
    with pytest.raises(ValueError, match="bootstrap_truncated"):
        r2.rollout(gru, list(range(B_ENVS)), hyps)
