"""Drop-in for the reference's ``a2c/updater.py``: ``Updater(net, hyps)`` with
``update_model(shared_data) -> info`` / ``bptt`` / ``save_model`` / ``new_lr`` / ``new_optim`` /
``print_statistics`` / ``log_statistics`` and the attributes ``net optim info norm hyps
is_discrete ret_mean ret_std`` (updater.py:9-229).

One ``update_model`` call enqueues, on one HIP stream and without host round trips until the
final read-back of five scalars:
  [hyps["bootstrap_truncated"]: final states -> critic forward -> a2c_trunc_bootstrap ->]
  fused GAE + returns scan -> model forward (N = n_rollouts*n_tsteps samples, or the BPTT unroll)
  -> advantage statistics -> fused loss forward+backward (continuous actions: Gaussian loss sums [-> all-reduce] ->
  Gaussian loss forward+backward; with hyps["gauss_loss"] = "exact" ONE launch, the per-sample Gaussian log-likelihood
  loss forward+backward, and no all-reduce) -> model backward into the flat gradient
  arena -> [RCCL all-reduce when sharded] -> grad-norm reduction -> fused clip + optimiser step (optim.OPTIMIZERS).
"""
import math
import sys

import torch

from . import ops, optim as fused_optim
from .parallel import Shard
from .utils import try_key


def recurrent_key(shared_data):
    return "h_states" in shared_data


GAUSS_LOSSES = ("reference", "exact")


def gauss_loss_mode(hyps, is_discrete=None):
    """hyps["gauss_loss"]: "reference" (the default, also when the key is absent: the reference's Gaussian loss, at parity)
    or "exact" (the per-sample log-likelihood loss, a2c_gauss_nll_fwd_bwd), for the nets with a
    Gaussian head only.  ValueError naming the key otherwise; is_discrete None = not known yet."""
    mode = try_key(hyps, "gauss_loss", "reference")
    if mode not in GAUSS_LOSSES:
        raise ValueError(f"a2c_amd: hyps['gauss_loss'] is 'reference' or 'exact', not {mode!r}")
    if mode == "exact" and is_discrete:
        raise ValueError("a2c_amd: hyps['gauss_loss'] = 'exact' is the loss of the continuous (Gaussian) nets: it needs "
                         "is_discrete=False")
    return mode


def ppo_settings(hyps):
    """hyps["ppo_epochs"] (int >= 1, default 1: today's one gradient step per rollout) and hyps["ppo_clip"] (float > 0,
    default 0.2) of the clipped multi-epoch update -> (epochs, clip); ValueError naming the key"""
    epochs, clip = try_key(hyps, "ppo_epochs", 1), try_key(hyps, "ppo_clip", 0.2)
    if isinstance(epochs, bool) or not isinstance(epochs, int) or epochs < 1:
        raise ValueError(f"a2c_amd: hyps['ppo_epochs'] is an int >= 1, not {epochs!r}")
    if isinstance(clip, bool) or not isinstance(clip, (int, float)) or not math.isfinite(clip) or clip <= 0:
        raise ValueError(f"a2c_amd: hyps['ppo_clip'] is a finite float > 0, not {clip!r}")
    return epochs, float(clip)


PPO_NETS = ("FCModel", "GRUFCModel")


def ppo_refusal(epochs, net_name, is_discrete, gauss_loss):
    """why hyps["ppo_epochs"] = epochs >= 2 cannot run on this net / loss (None: it can); net_name or is_discrete None = not
    known yet"""
    if epochs < 2:
        return None
    if net_name is not None and net_name not in PPO_NETS:
        return (f"a2c_amd: hyps['ppo_epochs'] >= 2 covers FCModel and GRUFCModel (the pixel nets' first forward comes from "
                f"the rollout's stash), not {net_name}")
    if is_discrete is not None and not is_discrete and gauss_loss != "exact":
        return ("a2c_amd: hyps['ppo_epochs'] >= 2 on a continuous net needs hyps['gauss_loss'] = 'exact': the reference's "
                "Gaussian loss is not a policy gradient, so it has no ratio to clip")
    return None


class _CutShard:
    """Shard stand-in used while capturing: every collective ends the graph being captured and starts the next"""

    def __init__(self, owner, real):
        self.o, self.real = owner, real
        self.rank, self.world, self.group = real.rank, real.world, real.group

    @property
    def active(self):
        return self.real.active

    def global_count(self, n):
        return self.real.global_count(n)

    def barrier(self):
        self.real.barrier()

    def allreduce_(self, t):
        if self.real.active:
            self.o._cut(t)
        return t


class _GraphedUpdate:
    def __init__(self, upd, shared_data):
        self.upd, self.graphs, self.colls = upd, [], []
        self.shared = shared_data
        self.fallbacks = 0          # replays that ran the eager update instead (the net's route had changed since the capture)
        net = upd.net
        torch.cuda.synchronize()
        dirty, route = net._dirty, net._route_state()
        # the route the captured launches take: the rollout's stash, lane masks, frame store and cells, and the switches
        self.route_sig = net._route_sig()
        real = upd.shard
        upd.shard = _CutShard(self, real)
        self._ctx = None
        try:
            self._begin()
            self.dev, self.n_global = upd._enqueue_update(shared_data)
            self._end()
        except BaseException:
            if self._ctx is not None:
                try:
                    self._ctx.__exit__(None, None, None)
                except Exception:      # noqa: BLE001
                    pass
            torch.cuda.synchronize()
            raise
        finally:
            upd.shard = real
        self.prep_sig = net._prep_sig() if hasattr(net, "_prep_sig") else ""
        # the capture itself executed nothing: the net is still in the state the rollout left it in (the optimiser step's
        # mark_dirty cleared all of the stash, not only its rows)
        net._dirty = dirty
        net._set_route_state(route)
        upd.optim._steps -= upd.ppo_epochs      # (one optimiser step per epoch was counted while capturing)

    def _stale_route(self):
        """the rollout before this replay left the net on another route than the captured one (a partial or split rollout: no
        stash; no ring kernel: no lane masks; ...): the captured launches would read what an EARLIER rollout left behind"""
        if self.upd.net._route_sig() == self.route_sig:
            return False
        self.fallbacks += 1
        if not getattr(self.upd, "_fallback_warned", False):
            self.upd._fallback_warned = True
            sys.stderr.write("a2c_amd: captured update replayed after a rollout that left the net on another route "
                             "(stash / lane masks / frame store / cells / switches): running the eager update instead\n")
        return True

    def _stale_prep(self):
        net = self.upd.net
        return (net._prep_sig() if hasattr(net, "_prep_sig") else "") != self.prep_sig

    def _begin(self):
        g = torch.cuda.CUDAGraph()
        self._ctx = ops.graph_capture(g)
        self._ctx.__enter__()
        self.graphs.append(g)

    def _end(self):
        self._ctx.__exit__(None, None, None)
        self._ctx = None

    def _cut(self, t):
        self._end()
        self.colls.append(t)
        self._begin()

    def replay(self):
        upd = self.upd
        if self._stale_route():
            return upd.update_model(self.shared)
        for i, g in enumerate(self.graphs):
            g.replay()
            if i < len(self.colls):
                upd.shard.allreduce_(self.colls[i])
        upd.optim._steps += upd.ppo_epochs
        upd.net.mark_dirty()
        # (the captured tail re-derived the inference weights: _enqueue_update's net._refresh -- unless the net derives more now)
        upd.net._dirty = self._stale_prep()
        return upd._finish_update(self.dev, self.n_global)

    __call__ = replay

    def replay_async(self):
        """replay() without the blocking read-back: -> token for Updater.collect(token) (the five scalars travel to a
        pinned host buffer behind the update on the stream; the caller may enqueue the NEXT rollout before collecting)"""
        upd = self.upd
        if self._stale_route():
            return upd.update_model_async(self.shared)
        for i, g in enumerate(self.graphs):
            g.replay()
            if i < len(self.colls):
                upd.shard.allreduce_(self.colls[i])
        upd.optim._steps += upd.ppo_epochs
        upd.net.mark_dirty()
        upd.net._dirty = self._stale_prep()
        return upd._post_async(self.dev, self.n_global)


class Updater:
    def __init__(self, net, hyps, shard=None):
        fused_optim.check_name(hyps["optim_type"])      # before any device work: an unsupported name is a ValueError
        self.net = net
        self.hyps = hyps
        self.is_discrete = hyps["is_discrete"]
        if bool(self.is_discrete) != bool(getattr(net, "is_discrete", True)):
            raise ValueError("a2c_amd: hyps['is_discrete'] does not match the net's is_discrete")
        self.gauss_loss = gauss_loss_mode(hyps, self.is_discrete)
        # time-limit truncation: the targets of a step whose episode the step limit alone ended
        # bootstrap from V(final state).  vecnorm: under hyps norm_obs the Runner's DeviceVecNorm (or a callable returning it;
        # train() sets it), whose apply-only path the final states pass through
        self.trunc = bool(try_key(hyps, "bootstrap_truncated", False))
        self.vecnorm = None
        if self.trunc and type(net).__name__ != "FCModel":
            raise ValueError("a2c_amd: bootstrap_truncated covers FCModel (the hidden row a recurrent net's final state needs "
                             f"is zeroed before anyone can read it), not {type(net).__name__}")
        self.shard = shard if shard is not None else Shard()
        # the clipped multi-epoch update: ppo_epochs == 1 is the one-step update, untouched
        self.ppo_epochs, self.ppo_clip = ppo_settings(hyps)
        why = ppo_refusal(self.ppo_epochs, type(net).__name__, self.is_discrete, self.gauss_loss)
        if why is None and self.ppo_epochs > 1 and self.shard.active:
            why = "a2c_amd: hyps['ppo_epochs'] >= 2 does not cover a sharded update (an active Shard)"
        if why is not None:
            raise ValueError(why)
        self.optim = self.new_optim(hyps["lr"])
        self.info = {}
        self.flat_scan_fallback = False     # last update: a slot did not end with done == 1 -> flat scans were used
        self.norm = 0
        self.ret_mean = None
        self.ret_std = None
        self._bufs = None

    # ------------------------------------------------------------------ helpers
    def _dev(self, t, dtype=torch.float32):
        dev = self.net._dev
        if t.device != dev or t.dtype != dtype or not t.is_contiguous():
            t = t.to(device=dev, dtype=dtype).contiguous()
        return t

    def _buffers(self, N):
        b = self._bufs
        if b is None or b["N"] != N:
            dev = self.net._dev
            b = dict(N=N,
                     advs=torch.empty(N, device=dev), rets=torch.empty(N, device=dev),
                     vals_c=torch.empty(N, device=dev),
                     stats=torch.zeros(8, dtype=torch.float64, device=dev),   # [adv sums 0:2 | loss sums 2:5 | ret 5:7]
                     scratch=ops.new_reduce_scratch(dev),     # this updater's ticket + partials (never shared, never born in a capture)
                     err=torch.zeros(1, dtype=torch.int32, device=dev),
                     out5=torch.zeros(5, dtype=torch.float64, device=dev),
                     host=torch.zeros(8, dtype=torch.float64).pin_memory() if torch.cuda.is_available() else None)
            if self.trunc:
                # the final states (filled in _bootstrap_truncated, where their row length is known), V of them, and the
                # corrected rewards / deltas: the Updater's own, shared_data is never written
                b.update(fin=None, vfin=torch.zeros(N, device=dev), rewards_tb=torch.empty(N, device=dev),
                         deltas_tb=torch.empty(N, device=dev))
            if not self.is_discrete and self.gauss_loss == "reference":
                # the six Gaussian loss sums (a2c_gauss_loss_sums), all-reduced when sharded
                b["gsums"] = torch.zeros(6, dtype=torch.float64, device=dev)
            if self.ppo_epochs > 1:
                # the behaviour policy's log-probability of every row (epoch 0 writes it), the five loss sums of the
                # clipped loss, and the update's scalars + [sum (1 - keep), sum ((r - 1) - log r)] for the ONE read-back
                b.update(logp_old=torch.zeros(N, dtype=torch.float64, device=dev),
                         ppo_sums=torch.zeros(5, dtype=torch.float64, device=dev),
                         out8=torch.zeros(8, dtype=torch.float64, device=dev))
            self._bufs = b
        return b

    # ------------------------------------------------------------------ the update
    def update_model(self, shared_data):
        """One A2C update (updater.py:53-137).  Everything up to the five scalars the reference reads
        back is enqueued on the stream without a host round trip (``_enqueue_update``: a launch-bound
        caller may capture that part into a hipGraph); ``_finish_update`` then syncs once."""
        return self._finish_update(*self._enqueue_update(shared_data))

    def _enqueue_update(self, shared_data):
        hyps, net, sh = self.hyps, self.net, self.shard
        net._ensure_device()
        net.req_grads(True)
        st = ops.stream()
        states = self._dev(shared_data["states"])
        rewards = self._dev(shared_data["rewards"]).reshape(-1)
        dones = self._dev(shared_data["dones"]).reshape(-1)
        deltas = self._dev(shared_data["deltas"]).reshape(-1)
        N = states.shape[0]
        if self.is_discrete:
            actions = self._dev(shared_data["actions"], torch.int64).reshape(-1)
        else:       # (N, n) float rows (training.py:89-92)
            actions = self._dev(shared_data["actions"]).reshape(N, net.output_space)
        T = int(hyps["n_tsteps"])
        if N % T:
            raise ValueError("len(states) is not a multiple of n_tsteps")
        R = N // T
        # global batch size: one blocking scalar all-reduce the first time a batch size is seen
        # (every rank steps with the same shapes, so the answer cannot change afterwards)
        cache = self.__dict__.setdefault("_n_global", {})
        if N not in cache:
            cache[N] = sh.global_count(N)
        n_global = cache[N]
        b = self._buffers(N)
        advs, rets, stats = b["advs"], b["rets"], b["stats"]
        if ops._TORCH_ABI_ON():     # A2C_TORCH_OPS=1: the launches below go through torch.ops.a2c_mi355x.abi_* (ops.TorchAbi),
            # which finds the tensor behind every address it is handed: tell it about the buffers that travel as raw rows
            for t in (states, rewards, dones, deltas, actions, net._arena.params, net._arena.grads,
                      shared_data.get("h_states") if recurrent_key(shared_data) else None, *[v for v in b.values() if torch.is_tensor(v)]):
                if t is not None and t.is_cuda:
                    ops.note_tensor(t)

        if self.trunc:
            rewards, deltas = self._bootstrap_truncated(shared_data, states, rewards, deltas, N, b, st)

        # advantages (gamma*lambda) and discounted returns (gamma) in one pass (updater.py:70-71, 86-88)
        with ops.span("gae_returns_scan"):
            ops.gae_returns(deltas, rewards, dones, hyps["gamma"] * hyps["lambda_"], hyps["gamma"], R, T, advs, rets,
                            err=b["err"], st=st)

        # forward pass (updater.py:73-80)
        recurrent = "h_states" in shared_data
        use_bptt = recurrent and bool(hyps["use_bptt"])
        if recurrent:
            h_states = self._dev(shared_data["h_states"])
            if use_bptt:
                net.bptt_forward(states, h_states, dones, R, T, "train", st)
            else:
                net._refresh(st)
                net._fwd(states.data_ptr(), states[0].numel(), N, "train", st, True, h_in=h_states)
        else:
            net._refresh(st)
            net._fwd(states.data_ptr(), states[0].numel(), N, "train", st, True)
        hb, logits, vals = net._heads("train", N)

        if hyps["use_nstep_rets"]:      # returns = advs + vals.data (updater.py:84)
            ops.copy_rows(vals.data_ptr(), vals.stride(0), b["vals_c"].data_ptr(), 1, N, 1, st)
            ops.add(advs, b["vals_c"], rets, st)
        if try_key(hyps, "norm_returns", False):
            self._norm_returns(rets, stats, n_global, st)

        adv_sums = None
        if hyps["norm_advs"]:           # (advs - mean)/(std + 1e-6) over the WHOLE batch (updater.py:97-98)
            adv_sums = stats[0:2]
            ops.moments(advs, adv_sums, st, scratch=b["scratch"])
            sh.allreduce_(adv_sums)

        if self.ppo_epochs > 1:
            return self._ppo_epochs(shared_data, states, dones, actions, advs, rets, adv_sums, N, R, T, n_global, b, st)

        db, dl, dv = net.dheads("train", N)
        if self.is_discrete:
            ops.loss_fwd_bwd(logits, vals, actions, advs, rets, adv_sums, n_global, try_key(hyps, "pi_coef", 1.0),
                             hyps["val_coef"], hyps["entr_coef"], dl, dv, stats[2:5], st, scratch=b["scratch"])
        elif self.gauss_loss == "exact":
            # the per-sample log-likelihood loss: every row's gradient from that row and the advantage statistics alone, so
            # one launch and no collective (the three loss sums travel in the gradient arena's tail below)
            ops.gauss_nll_fwd_bwd(logits, vals, actions, advs, rets, adv_sums, n_global, net.output_space,
                                  try_key(hyps, "pi_coef", 1.0), hyps["val_coef"], hyps["entr_coef"], dl, dv, stats[2:5], st,
                                  scratch=b["scratch"])
        else:
            # the Gaussian loss needs batch-wide sums before any gradient (mse and K of the mu gradient): two launches,
            # the sums all-reduced in between when sharded (a capture is cut there, like at the advantage moments)
            n, gs = net.output_space, b["gsums"]
            ops.gauss_loss_sums(logits, vals, actions, advs, rets, adv_sums, n_global, n, gs, st, scratch=b["scratch"])
            sh.allreduce_(gs)
            ops.gauss_loss_fwd_bwd(logits, vals, actions, advs, rets, adv_sums, gs, n_global, n,
                                   try_key(hyps, "pi_coef", 1.0), hyps["val_coef"], hyps["entr_coef"], dl, dv, stats[2:5], st)

        # backward into the flat gradient arena
        if use_bptt:
            net.bptt_backward(states, dones, R, T, "train", st)
        else:
            net._bwd(states.data_ptr(), states[0].numel(), N, "train", st)
        net._arena.attach_grads()
        if sh.active:                   # ONE all-reduce over xGMI per update: gradients + the three loss sums in its tail
            tail = net._arena.grad_tail()
            tail[:3].copy_(stats[2:5])                      # reporting only (updater.py:134-136): fp32 is plenty
            sh.allreduce_(net._arena.reduce_span())
            stats[2:5].copy_(tail[:3])

        # clip_grad_norm_ + optimiser step (updater.py:129-132), fused
        with ops.span("clip_optimizer"):
            self.optim.step(max_norm=hyps["max_norm"], st=st)
        self.optim.zero_grad()

        # the weights just changed: re-derive what the NEXT rollout needs from them (conv fragments, composed heads) here, at
        # the tail of the update's stream work (inside its hipGraph when captured), not on the host path between the
        # read-back below and the rollout kernel's launch, where the GPU would sit idle behind ~50 us of Python + 5 launches
        net._refresh(st)
        # five scalars for the host (the reference's .item() calls, updater.py:134-136), gathered by one kernel
        ops.check(ops.lib().a2c_pack_update_scalars(stats[2:5].data_ptr(), self.optim.grad_norm().data_ptr(),
                                                    b["err"].data_ptr(), b["out5"].data_ptr(), st), "a2c_pack_update_scalars")
        return b["out5"], n_global

    def _ppo_epochs(self, shared_data, states, dones, actions, advs, rets, adv_sums, N, R, T, n_global, b, st):
        """hyps["ppo_epochs"] = K >= 2, from behind the advantage moments of _enqueue_update on: K
        times [clipped loss -> backward -> clip + optimiser step] on the same rows, advantages and returns.  Epoch 0 uses
        the forward that is already there and RECORDS every row's log-probability (the parameters are the rollout's: its
        ratio is 1 and its gradient the policy gradient); the later epochs run the forward again and read it."""
        hyps, net = self.hyps, self.net
        recurrent = "h_states" in shared_data
        use_bptt = recurrent and bool(hyps["use_bptt"])
        h_states = self._dev(shared_data["h_states"]) if recurrent else None
        S = states[0].numel()
        sums = b["ppo_sums"]
        coefs = (try_key(hyps, "pi_coef", 1.0), hyps["val_coef"], hyps["entr_coef"], self.ppo_clip)
        for epoch in range(self.ppo_epochs):
            if epoch:
                if use_bptt:
                    net.bptt_forward(states, h_states, dones, R, T, "train", st)
                elif recurrent:
                    net._refresh(st)
                    net._fwd(states.data_ptr(), S, N, "train", st, True, h_in=h_states)
                else:
                    net._refresh(st)
                    net._fwd(states.data_ptr(), S, N, "train", st, True)
            hb, logits, vals = net._heads("train", N)
            db, dl, dv = net.dheads("train", N)
            if self.is_discrete:
                ops.ppo_loss_fwd_bwd(logits, vals, actions, advs, rets, adv_sums, n_global, *coefs, epoch == 0, b["logp_old"],
                                     dl, dv, sums, st, scratch=b["scratch"])
            else:
                ops.gauss_ppo_fwd_bwd(logits, vals, actions, advs, rets, adv_sums, n_global, net.output_space, *coefs,
                                      epoch == 0, b["logp_old"], dl, dv, sums, st, scratch=b["scratch"])
            if use_bptt:
                net.bptt_backward(states, dones, R, T, "train", st)
            else:
                net._bwd(states.data_ptr(), S, N, "train", st)
            net._arena.attach_grads()
            with ops.span("clip_optimizer"):
                self.optim.step(max_norm=hyps["max_norm"], st=st)
            self.optim.zero_grad()
        net._refresh(st)
        # the last epoch's five scalars as in _enqueue_update, the clip count and the KL sum behind them: one vector, one read
        out = b["out8"]
        ops.check(ops.lib().a2c_pack_update_scalars(sums.data_ptr(), self.optim.grad_norm().data_ptr(), b["err"].data_ptr(),
                                                    out.data_ptr(), st), "a2c_pack_update_scalars")
        out[5:7].copy_(sums[3:5])
        return out, n_global

    def _bootstrap_truncated(self, shared_data, states, rewards, deltas, N, b, st):
        """hyps["bootstrap_truncated"], all on the update's stream, before the scan: the state every
        row's episode would have gone on from (a2c_final_states), under norm_obs through the normaliser's apply-only path --
        the block AS IT STANDS AT UPDATE TIME, not as it stood at step t: what evaluation does --, one forward through a
        workspace of its own ("vfin": the "train" forward that follows is not disturbed) for V of them, and
        a2c_trunc_bootstrap: rewards / deltas + gamma * truncs * V into this Updater's buffers -> (rewards, deltas) for the
        scan.  The scan cuts at done, so the closing step's reward and delta carry the whole correction"""
        if "h_states" in shared_data:
            raise ValueError("a2c_amd: bootstrap_truncated covers feed-forward rollouts (no shared_data['h_states'])")
        for name in ("truncs", "final_obs"):
            if name not in shared_data:
                raise ValueError(f"a2c_amd: bootstrap_truncated needs shared_data[{name!r}] (the Runner fills it)")
        net, hyps = self.net, self.hyps
        C, S = int(states.shape[1]), int(states[0].numel())
        HW = S // C
        truncs = self._dev(shared_data["truncs"]).reshape(-1)
        final_obs = self._dev(shared_data["final_obs"]).reshape(N, HW)
        if b["fin"] is None or tuple(b["fin"].shape) != (N, S):
            b["fin"] = torch.zeros((N, S), device=net._dev)
        fin = b["fin"]
        ops.final_states(states, final_obs, C, HW, N, fin, st)
        if try_key(hyps, "norm_obs", False):
            vn = self.vecnorm() if callable(self.vecnorm) else self.vecnorm
            if vn is None:
                raise ValueError("a2c_amd: bootstrap_truncated under norm_obs normalises the final states by the Runner's "
                                 "block: set Updater.vecnorm = runner.vecnorm")
            vn.launch(N, 0, out_ptr=fin.data_ptr(), out_stride=S, C=C, update=False, st=st)
        net._refresh(st)
        vals = net._fwd(fin.data_ptr(), S, N, "vfin", st, False)["vals"]
        ops.copy_rows(vals.data_ptr(), vals.stride(0), b["vfin"].data_ptr(), 1, N, 1, st)
        ops.trunc_bootstrap(rewards, deltas, truncs, b["vfin"], hyps["gamma"], N, b["rewards_tb"], b["deltas_tb"], st)
        return b["rewards_tb"], b["deltas_tb"]

    def capture_update(self, shared_data):
        """The enqueue half of update_model as hipGraphs: ONE graph on a single GPU; with a sharded update the captured
        stream is cut at every collective (advantage moments, gradient arena) -- graph, RCCL all-reduce on the stream,
        graph, ... -- so that N-GPU updates are not ~40 eager launches either and no collective sits inside a capture.
        Returns a callable ``replay() -> info`` (same effect as update_model on the same buffers); the caller must
        have run one eager update_model on these buffers first (workspaces, tuners, one-time hipMalloc / hipMemset of
        the GEMM and conv launchers: none of that is legal inside a capture).  The captured launches follow the route the
        preceding rollout left in the net (net._route_sig: stash, lane masks, frame store, cells, switches); a replay after a
        rollout that left another route runs the eager update_model instead (``.fallbacks`` counts those, one warning on
        stderr), so a replay never reads the activations of an earlier rollout.  Every rank of a sharded update decides
        alike when its rollouts were alike."""
        if not getattr(self.optim, "capture_safe", False):
            # Adam's bias correction (and the other step-dependent scalars: NAdam's mu, ASGD's eta, ...) takes the step
            # count as a KERNEL ARGUMENT: a replay would apply the captured step's values for ever.  With
            # hyps["optim_capturable"] the count and the scalars live on the device and the optimiser is capture_safe.
            raise RuntimeError(f"a2c_amd: {type(self.optim).__name__}.step cannot be captured into a hipGraph "
                               "(its step count is a kernel argument); use update_model, or hyps['optim_capturable'] = True")
        if self._bufs is None:
            raise RuntimeError("a2c_amd: capture_update needs one eager update_model on these buffers first")
        return _GraphedUpdate(self, shared_data)

    def update_model_async(self, shared_data):
        """update_model without the blocking read-back of the five scalars: everything is enqueued, the scalars go to a
        pinned host buffer behind the update on the stream; ``collect(token)`` waits for THAT copy only and returns the info
        dict.  Lets a driver enqueue the next rollout (which needs nothing from the host) before it looks at the losses."""
        return self._post_async(*self._enqueue_update(shared_data))

    def _post_async(self, dev_vec, n_global):
        hb = self.__dict__.setdefault("_host_ring", [torch.zeros(8, dtype=torch.float64).pin_memory() for _ in range(4)])
        i = self.__dict__["_host_i"] = (self.__dict__.get("_host_i", -1) + 1) % len(hb)
        hb[i][:dev_vec.numel()].copy_(dev_vec, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return (ev, hb[i], n_global)

    def collect(self, token):
        ev, host, n_global = token
        ev.synchronize()
        return self._finish_host(host, n_global)

    def _finish_update(self, dev_vec, n_global):
        return self._finish_host(dev_vec.cpu(), n_global)

    def _finish_host(self, host, n_global):
        hyps = self.hyps
        # host[4] != 0: a slot did not end with done == 1 (not Runner data, runner.py:244); the scans then ran in
        # the reference's flat form on the device (a2c_gae_returns_fused), so the update is still the reference's
        self.flat_scan_fallback = bool(int(host[4]))
        s_pi, s_val, s_ent = (float(host[i]) for i in range(3))
        pi_loss = try_key(hyps, "pi_coef", 1.0) * -(s_pi / n_global)
        val_loss = hyps["val_coef"] * (s_val / n_global)
        entr_loss = -hyps["entr_coef"] * (s_ent / n_global)
        self.norm = float(host[3])
        self.info = {"Loss": pi_loss + val_loss - entr_loss, "Pi_Loss": pi_loss, "ValLoss": val_loss,
                     "Entropy": entr_loss, "GradNorm": self.norm}
        if self.ppo_epochs > 1:         # the last epoch's: the share of rows the clip stopped, and mean((r - 1) - log r)
            self.info["ClipFrac"] = float(host[5]) / n_global
            self.info["ApproxKL"] = float(host[6]) / n_global
        return self.info

    def _norm_returns(self, rets, stats, n_global, st):
        """EMA-normalised returns (updater.py:89-96, default off): needs the batch mean/std on the
        host to update the running values, hence one extra read-back."""
        sums = stats[5:7]
        ops.moments(rets, sums, st, scratch=self._bufs["scratch"])
        self.shard.allreduce_(sums)
        s0, s1 = (float(v) for v in sums.cpu())
        mean = s0 / n_global
        std = max((s1 - n_global * mean * mean) / (n_global - 1), 0.0) ** 0.5
        if self.ret_mean is None:
            self.ret_mean, self.ret_std = mean, std
        else:
            self.ret_mean = 0.01 * mean + 0.99 * self.ret_mean
            self.ret_std = 0.01 * std + 0.99 * self.ret_std
        # encode (ret_mean, ret_std) as moment sums of a virtual population so the same kernel applies them
        n = float(n_global)
        fake = torch.tensor([self.ret_mean * n, (self.ret_std ** 2) * (n - 1) + n * self.ret_mean ** 2],
                            dtype=torch.float64, device=rets.device)
        ops.normalize(rets, rets, fake, n_global, 1e-6, st)

    def bptt(self, states, h_states, dones):
        """updater.py:139-169: unrolled recurrent forward; returns (vals (N,), logits (N,A)), or (vals (N,), (mu (N,n),
        sigma (N,n))) for a continuous net."""
        hyps, net = self.hyps, self.net
        net._ensure_device()
        R, T = int(hyps["n_rollouts"]), int(hyps["n_tsteps"])
        st = ops.stream()
        vals, logits = net.bptt_forward(self._dev(states), self._dev(h_states), self._dev(dones).reshape(-1), R, T,
                                        "train", st)
        if net.is_discrete:
            return vals.clone(), logits.clone()
        mu, sigma = net._policy_out(logits, "train", R * T, st)
        return vals.clone(), (mu.clone(), sigma.clone())

    def gae(self, rewards, values, next_vals, dones, gamma, lambda_):
        """updater.py:172-189 (unused by the reference's own loop; kept for API parity)."""
        from .utils import discount
        deltas = rewards + gamma * next_vals * (1 - dones) - values
        return discount(deltas, dones, gamma * lambda_)

    # ------------------------------------------------------------------ bookkeeping API
    def print_statistics(self):
        nums = {k: (v.item() if isinstance(v, torch.Tensor) else v) for k, v in self.info.items()}
        print(" – ".join(k + ": " + str(round(v, 5)) for k, v in sorted(nums.items())))

    def log_statistics(self, log, T, reward, avg_action, best_avg_rew):
        nums = {k: (v.item() if isinstance(v, torch.Tensor) else v) for k, v in self.info.items()}
        arr = [k + ": " + (str(round(v, 5)) if "ntropy" not in k else str(v)) for k, v in nums.items()]
        arr += ["EpRew: " + str(reward), "AvgAction: " + str(avg_action), "BestRew:" + str(best_avg_rew)]
        log.write("Step:" + str(T) + " – " + " – ".join(arr) + "\n")
        log.flush()

    def save_model(self, net_file_name, optim_file_name):
        torch.save(self.net.state_dict(), net_file_name)
        if optim_file_name is not None:
            torch.save(self.optim.state_dict(), optim_file_name)

    def new_lr(self, new_lr):
        # like the reference: a new optimiser that then loads the old state (which, as in the
        # reference, also restores the old lr: updater.py:221-224)
        new_optim = self.new_optim(new_lr)
        new_optim.load_state_dict(self.optim.state_dict())
        self.optim = new_optim

    def new_optim(self, lr):
        cls = fused_optim.check_name(self.hyps["optim_type"])
        # hyps["optim_capturable"]: torch's capturable=True for the Adam family (step count and bias corrections on the
        # device, so capture_update / replay work); the other optimisers are capture-safe as they are and ignore it
        if try_key(self.hyps, "optim_capturable", False) and cls._kind is not None:
            return cls(self.net, lr=lr, capturable=True)
        return cls(self.net, lr=lr)
