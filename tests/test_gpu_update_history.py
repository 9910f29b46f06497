"""-m gpu: an update is a function of its buffers and the weights, not of the rollout that filled the buffers.

The update also reads what the preceding rollout left in the net: the stash of conv activations (and ConvModel's embedding
rows), A3CModel's lane masks / mask bits (ring kernel only), the single-frame store, GRUModel's BPTT cells.  A captured
update records whichever of those routes was live at capture; a replay after a rollout that left another route must not
read what an EARLIER rollout left there (it falls back to the eager update).  Rollout histories that fill the same buffers
with the same values but leave different net state:
  full    one Runner.rollout over all slots (the stash, and with the ring kernel the lane masks, are live)
  split   two Runner.rollout calls over complementary halves of the slot list (same buffers, no stash)
  noring  A2C_NO_RING=1 (A3CModel): the per-step body, stash without lane masks
  nocell  A2C_NO_CELL_STASH=1 (GRUModel): stash without the BPTT cells
  nostash A2C_NO_STASH=1 during the rollout (no stash, the frame store is still written)
The runner plays a slot list in rounds of n_envs slots, slot k of a round by env k: with n_envs = half the slots, `full`
plays the same two rounds, env for env, as `split` does -- the buffers are identical, only the net state differs.  The
cell stash (all slots in lock-step) and the frame store need n_envs = all slots: those cases use `nocell` / `nostash`."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import a2c_oracle as O  # noqa: E402
from cases import U8FakeEnv, base_hyps, hashf  # noqa: E402
from test_gpu_models import _datas, make_net  # noqa: E402
from test_gpu_ingest import _pool  # noqa: E402

DEV = "cuda"
BUFS = ("states", "actions", "rewards", "dones", "deltas")


class _Engine:
    """rollouts with a chosen history over n_envs = B / E envs (E rounds), and an Updater"""

    def __init__(self, kind, ingest, hyps, ekws, usd, B, T, A, ss, h, pool=None):
        from a2c_amd.runner import Runner
        from a2c_amd.updater import Updater
        self.net = make_net(kind, ss, A, h)
        self.D = _datas(B * T, ss, self.net.is_recurrent, h=h, actions_on_host=False)
        self.rnd = [0]
        self.pool = pool if pool is not None else _pool(U8FakeEnv, ekws, 2, pong=True)
        self.r = Runner(self.D, hyps, None, None, None, env_pool=self.pool, ingest=ingest,
                        uniform_fn=lambda t, Bn, env0: usd[self.rnd[0], t, env0:env0 + Bn].contiguous())
        self.upd = Updater(self.net, hyps)
        self.hyps, self.B, self.E = hyps, B, self.pool.n_envs if pool is not None else len(ekws)
        self.g = None

    def rollout(self, k, hist, monkeypatch):
        self.rnd[0] = k
        sw = {"noring": "A2C_NO_RING", "nocell": "A2C_NO_CELL_STASH", "nostash": "A2C_NO_STASH"}.get(hist)
        if sw:
            monkeypatch.setenv(sw, "1")
        try:
            if hist == "split":
                self.r.rollout(self.net, list(range(self.E)), self.hyps)
                self.r.rollout(self.net, list(range(self.E, self.B)), self.hyps)
            else:
                self.r.rollout(self.net, list(range(self.B)), self.hyps)
            self.r.finish()
        finally:
            if sw:
                monkeypatch.delenv(sw)

    def close(self):
        self.r.close()


def _oracle_net(kind, hyps, ekws, us, n_ep, B, T, ss, A, h):
    """the oracle's SlotRunner + OracleUpdater over the same schedule: env e plays slots e, e + E, ... of every epoch with the
    uniforms of env e (Runner: uniform_fn(t, B, env0) per round)"""
    onet = O.OracleNet(kind, ss, A, h)
    oupd = O.OracleUpdater(onet, hyps)
    E, N = len(ekws), B * T
    Do = dict(states=torch.zeros(N, *ss), deltas=torch.zeros(N), rewards=torch.zeros(N), dones=torch.zeros(N),
              actions=torch.zeros(N).long())
    if onet.is_recurrent:
        Do["h_states"] = torch.zeros(N, h)
    runners = []
    for e in range(E):
        seq = iter([float(us[k, t, e]) for k in range(n_ep) for _ in range(B // E) for t in range(T)])
        sr = O.SlotRunner(O.FakeEnv(**ekws[e]), Do, hyps, uniform_fn=lambda seq=seq: next(seq))
        sr.start(onet)
        runners.append(sr)
    for k in range(n_ep):
        for r0 in range(0, B, E):
            for e in range(E):
                runners[e].rollout(onet, r0 + e)
        oupd.update_model(Do)
    return onet


# name: kind, ingest, bptt, B (slots), T, n_envs, capture history, replay histories, hyps extra, oracle
CASES = {
    "a3c-stream": ("A3CModel", "zero-copy", False, 32, 128, 16, ["split", "full", "noring", "split"], {}, False),
    "a3c-small": ("A3CModel", "zero-copy", False, 4, 5, 2, ["split", "full", "noring", "split"], {}, True),
    "gru-bptt": ("GRUModel", "relay", True, 4, 5, 2, ["split", "full", "split"], {}, True),
    "gru-cells": ("GRUModel", "relay", True, 4, 5, 4, ["nocell", "full", "nocell"], {}, True),
    "conv-frames": ("ConvModel", "relay", False, 4, 5, 4, ["nostash", "full", "nostash"], dict(frame_store=True), True),
}
# capture after `full`; and capture after the case's stash-less history, replays after `full`
SCHEDULES = [(c, "full") for c in CASES] + [(c, CASES[c][6][0]) for c in CASES if c != "gru-cells"]


@pytest.mark.parametrize("case,cap", SCHEDULES, ids=[f"{c}-capture_after_{h}" for c, h in SCHEDULES])
def test_replayed_update_equals_eager_across_rollout_histories(case, cap, monkeypatch):
    """epoch 0: `full` + eager update on both twins; epoch 1: history `cap`, capture_update + replay on one twin, eager
    update_model on the other; later epochs: the other histories, replay_async / replay vs update_model.  After every update
    the five infos, every parameter and the optimiser's state are bit-identical to the eager twin's; a third engine plays
    `full` throughout and pins that every history left the same buffers.  A replay after a history of the capture's own
    kind runs the graph (no fallback).  The final weights against the oracle (tolerances of the timed-path test)."""
    from a2c_amd import ops
    kind, ingest, bptt, B, T, E, hists, extra, with_oracle = CASES[case]
    if cap != "full":
        hists = ["full", cap, "full"]
    sched = ["full", cap] + hists
    n_ep = len(sched)
    A, ss, h = 3, (4, 84, 84), 256
    ekws = [dict(env_id=j, rew_period=2 + j % 2, done_period=4 + j) for j in range(E)]
    hyps = base_hyps(env_type="FakePong-v0", n_tsteps=T, n_rollouts=B, action_shift=0, n_envs=E, lr=1e-3,
                     optim_type="RMSprop", use_bptt=bptt, h_size=h, **extra)
    us = torch.from_numpy(hashf(n_ep * T * E, 4177, 0, 1).reshape(n_ep, T, E))
    usd = us.to(DEV)
    eg = _Engine(kind, ingest, hyps, ekws, usd, B, T, A, ss, h)         # graphed
    ee = _Engine(kind, ingest, hyps, ekws, usd, B, T, A, ss, h)         # eager twin, same histories
    ef = _Engine(kind, ingest, hyps, ekws, usd, B, T, A, ss, h)         # `full` throughout, eager
    if case == "a3c-stream":       # the streaming batch: lane masks and the bf16 x 6 conv2 backward-data are on the route
        assert ops.conv_bwd_data_lanemask_supported(eg.net._c2.d, B * T)
    same_w = True                  # ef's weights == the twins' (eager updates that do not depend on the history)
    try:
        for k, hist in enumerate(sched):
            for e in (eg, ee):
                e.rollout(k, hist, monkeypatch)
            ef.rollout(k, "full", monkeypatch)
            for n in BUFS:
                assert torch.equal(eg.D[n], ee.D[n]), (k, hist, n)
                if same_w and not (n == "deltas" and hist == "noring"):
                    assert torch.equal(eg.D[n], ef.D[n]), (k, hist, n)
            if same_w and hist == "noring":
                # the per-step body's values round differently from the ring kernel's: the deltas agree to fp32 noise only
                torch.testing.assert_close(eg.D["deltas"], ef.D["deltas"], rtol=1e-5, atol=1e-6)
            if hist == "full":
                assert eg.net._stash is not None                        # the stash route is live after `full`
                if case == "a3c-stream":
                    assert eg.net._stash_lm
                if case == "conv-frames":
                    assert eg.net._stash_frames is not None
                if case == "gru-cells":
                    assert eg.net._cells_done == T - 1
            if hist in ("split", "nostash"):
                assert eg.net._stash is None
            if k == 0:
                gi = eg.upd.update_model(eg.D)
            else:
                fb0 = getattr(eg.g, "fallbacks", 0)
                if eg.g is None:
                    eg.g = eg.upd.capture_update(eg.D)
                    assert len(eg.g.graphs) == 1 and not eg.g.colls
                gi = eg.g.replay() if k % 2 else eg.upd.collect(eg.g.replay_async())
            ei = ee.upd.update_model(ee.D)
            fi = ef.upd.update_model(ef.D)
            for name in ei:
                assert gi[name] == ei[name], (k, hist, name, gi, ei)
            assert eg.upd.optim._steps == ee.upd.optim._steps == k + 1
            for (n, p), (_, q) in zip(eg.net.named_parameters(), ee.net.named_parameters()):
                assert torch.equal(p, q), (k, hist, n, float((p - q).abs().max()))
            for a, b in zip(eg.upd.optim._flat.values(), ee.upd.optim._flat.values()):
                assert torch.equal(a, b), (k, hist)
            if k > 0:        # the captured route: the graph ran; another route: the eager update ran instead
                assert eg.g.fallbacks == fb0 + int(_route_differs(case, cap, hist)), (k, hist, eg.g.fallbacks)
            if k == 3:
                w4 = [p.detach().clone() for p in eg.net.parameters()]
            if same_w:
                diff = [n for (n, p), (_, q) in zip(ee.net.named_parameters(), ef.net.named_parameters()) if not torch.equal(p, q)]
                if diff:
                    # (the no-stash route recomputes the forward: other fp32 roundings of the activations and heads; the
                    # fp64 comparison of every history is test_eager_a3c_update_is_independent_of_the_rollout_history)
                    print(f"[{case}] epoch {k}: eager update after `{hist}` != after `full` in {diff} "
                          f"(infos {ei} vs {fi})")
                    same_w = False
        if with_oracle:         # after 4 updates, as test_graphed_update_replays_equal_eager_updates_and_the_oracle
            onet = _oracle_net(kind, hyps, ekws, us, 4, B, T, ss, A, h)
            for (n, _), p, (n2, q) in zip(eg.net.named_parameters(), w4, onet.named_parameters()):
                assert n == n2
                d = (p.detach().cpu() - q.detach()).abs()
                assert float(d.max()) <= 4e-2 and float(d.mean()) <= 2e-4, (n, float(d.max()), float(d.mean()))
    finally:
        for e in (eg, ee, ef):
            e.close()


def _route_differs(case, cap, hist):
    """does `hist` leave another route than `cap` (stash rows, lane masks, cells)?  Small A3CModel batches have no lane
    masks, so `noring` is `full` there"""
    def route(hh):
        if hh in ("split", "nostash"):
            return "none"
        if hh == "noring" and case == "a3c-stream":
            return "stash"
        if hh == "nocell":
            return "stash"
        return "stash+lm" if case == "a3c-stream" else ("stash+cells" if case == "gru-cells" else "stash")
    return route(cap) != route(hist)


def test_route_table_of_the_schedules():
    assert _route_differs("a3c-stream", "full", "noring") and not _route_differs("a3c-small", "full", "noring")
    assert _route_differs("gru-cells", "full", "nocell") and not _route_differs("gru-bptt", "split", "split")


def test_continuous_fc_control_never_falls_back(monkeypatch):
    """Continuous FCModel has no stash: every history leaves the same route, every replay runs the graph, bit-identical to
    the eager twin."""
    import cont_cases as CC
    import a2c_amd
    from a2c_amd.runner import HostEnvPool, Runner
    from a2c_amd.updater import Updater
    n, h, B, T, E = 2, 16, 4, 5, 2
    sched = ["full", "full", "split", "full", "split"]
    eps = torch.from_numpy(hashf(len(sched) * T * E * n, 991, -1, 1).reshape(len(sched), T, E, n)).cuda()

    def engine():
        net = a2c_amd.FCModel(list(CC.STATE_SHAPE), n, h_size=h, is_discrete=False)
        net.load_state_dict(CC.state_dict("FCModel", n, h, CC.UPDATE_RAW_BIAS[n]))
        net = net.cuda()
        D = dict(states=torch.zeros(B * T, *CC.STATE_SHAPE, device=DEV), deltas=torch.zeros(B * T, device=DEV),
                 rewards=torch.zeros(B * T, device=DEV), dones=torch.zeros(B * T, device=DEV),
                 actions=torch.zeros(B * T, n, device=DEV))
        hyps = CC.cont_hyps(n_tsteps=T, n_rollouts=B, n_envs=E, optim_type="RMSprop", h_size=h, lr=1e-3)
        rnd = [0]
        envs = [CC.ContEnv(n, env_id=j, done_period=4 + j, prepped=True) for j in range(E)]
        r = Runner(D, hyps, None, None, None, env_pool=HostEnvPool(envs),
                   normal_fn=lambda t, Bn, e0: eps[rnd[0], t, e0:e0 + Bn])
        return net, D, hyps, rnd, r, Updater(net, hyps)

    (ng, Dg, hyps, rg, r_g, ug), (ne, De, _, re_, r_e, ue) = engine(), engine()
    g = None
    for k, hist in enumerate(sched):
        for net, D, rnd, r in ((ng, Dg, rg, r_g), (ne, De, re_, r_e)):
            rnd[0] = k
            if hist == "split":
                r.rollout(net, list(range(E)), hyps)
                r.rollout(net, list(range(E, B)), hyps)
            else:
                r.rollout(net, list(range(B)), hyps)
        for nm in BUFS:
            assert torch.equal(Dg[nm], De[nm]), (k, nm)
        if k == 0:
            gi = ug.update_model(Dg)
        else:
            g = g or ug.capture_update(Dg)
            gi = g.replay()
        ei = ue.update_model(De)
        assert gi == ei, (k, gi, ei)
        for p, q in zip(ng.parameters(), ne.parameters()):
            assert torch.equal(p, q), k
    assert g.fallbacks == 0


def test_eager_a3c_update_is_independent_of_the_rollout_history(monkeypatch):
    """A3CModel at streaming batch (32 x 128, 16 envs): update_model on the same states and weights after a `full` (ring:
    stash + lane masks + mask bits), a `noring` (stash, float mask) and a `split` rollout (no stash: the update runs its own
    forward).  Bit-identity across the three is not possible: the ring kernel's values (-> deltas) round differently from the
    per-step body's, and without the stash the update's forward recomputes the activations with the layered conv kernels and
    the heads through proj_matrx instead of the composed matrix.  So: states, actions and dones bit for bit, rewards and
    deltas to fp32 noise, the per-tensor gradient differences printed (pytest -s), and EVERY history's update against the fp64
    autograd gradient of the reference loss on its own recorded buffers, as
    test_full_size_headline_update_matches_the_oracle_updater does."""
    from test_gpu_timed_path import _compare_full_update, _oracle_updates_fp32_and_fp64
    from a2c_amd import ops
    from a2c_amd.hostpool import ThreadEnvPool
    from a2c_amd.synthetic import TapeEnv
    kind, B, T, E, A, ss, h = "A3CModel", 32, 128, 16, 3, (4, 84, 84), 256
    # the headline test's tape envs (dense gradients in every layer); each env plays two slots of T steps
    hyps = base_hyps(env_type="Pong-synthetic", n_tsteps=T, n_rollouts=B, action_shift=0, n_envs=E, optim_type="RMSprop")
    usd = torch.from_numpy(hashf(T * E, 5113, 0, 1).reshape(1, T, E)).to(DEV)
    res = {}
    for hist in ("full", "noring", "split"):
        envs = [TapeEnv(env_id=j, length=2 * T + 1, p_done=1.0 / 100) for j in range(E)]
        pool = ThreadEnvPool.from_tape_envs(envs, n_threads=4, pong=True, frame_bits=True)
        e = _Engine(kind, "zero-copy", hyps, None, usd, B, T, A, ss, h, pool=pool)
        try:
            assert ops.conv_bwd_data_lanemask_supported(e.net._c2.d, B * T)
            e.rollout(0, hist, monkeypatch)
            assert (e.net._stash is not None) == (hist != "split") and bool(e.net._stash_lm) == (hist == "full")
            info = e.upd.update_model(e.D)
            torch.cuda.synchronize()
            res[hist] = (info, {n: e.net.G(n).clone() for n, _ in e.net.named_parameters() if n not in e.net._unused_params},
                         {k: v.cpu().clone() for k, v in e.D.items()}, e.net)
        finally:
            e.close()
    f_info, f_g, f_D, _ = res["full"]
    for hist in ("noring", "split"):
        info, gr, D, _ = res[hist]
        for k in ("states", "actions", "dones"):
            assert torch.equal(D[k], f_D[k]), (hist, k)
        # (on these tape envs the per-step body's rewards, like its values, are not bit-identical to the ring kernel's)
        for k in ("rewards", "deltas"):
            torch.testing.assert_close(D[k], f_D[k], rtol=1e-5, atol=1e-6)
        print(f"[{hist} vs full] " + ", ".join(
            f"{n}: {float((gr[n] - f_g[n]).abs().max()) / max(float(f_g[n].abs().max()), 1e-30):.1e}" for n in gr))
    for hist, (info, _, D, net) in res.items():
        onet = O.OracleNet(kind, ss, A, h)
        oinfo, g32, oinfo64, g64 = _oracle_updates_fp32_and_fp64(kind, ss, A, h, O.OracleUpdater(onet, hyps), D, hyps, monkeypatch)
        _compare_full_update(net, info, onet, oinfo, g32, oinfo64, g64, hyps["max_norm"])
