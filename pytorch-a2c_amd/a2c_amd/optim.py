"""Fused clip + optimiser steps over the flat parameter arena (updater.py:129-132, 226-229).

Every optimiser here is a ``torch.optim.Optimizer`` subclass whose ``state_dict()`` has the layout of the
``torch.optim`` class of the same name (param indices follow ``net.parameters()``, per-parameter ``step`` and the
rule's state), so ``optim.p`` checkpoints (training.py:127-128, updater.py:218-219) load either way.  The state
tensors are views into flat HBM buffers parallel to the net's arena; one kernel launch updates every parameter.
Settings are torch's defaults apart from ``lr`` (the reference only ever passes ``lr``): RMSprop / Adam and the
other torch optimisers that step without a closure (``OPTIMIZERS``).  A loaded param_group that asks for something
the kernels do not implement (momentum, maximize, amsgrad, weight decay outside AdamW, ...) raises ``ValueError``.

``capturable=True`` (Adam, AdamW, Adamax, NAdam, RAdam, ASGD; torch's flag of the same name) keeps the step count and the
step-dependent scalars in a device block (``ops.optim_block_*``): ``step()`` is then [advance, step] with no step-dependent
kernel argument, so ``Updater.capture_update`` can replay it.  The mode is fixed at construction.
"""
import numpy as np
import torch

from . import ops


def _f32(x):
    """a python float rounded to fp32, as torch stores a 0-d float32 state tensor"""
    return float(np.float32(x))


def nadam_mu_product(mu_product, step, beta1, momentum_decay):
    """torch's fp32 ``mu_product *= mu`` at the 1-based ``step``: the python-float mu is rounded to fp32, then the product"""
    mu = beta1 * (1.0 - 0.5 * (0.96 ** (step * momentum_decay)))
    return _f32(mu_product * _f32(mu))


def asgd_eta_mu(step, lr, lambd, alpha, t0):
    """the fp32 (eta, mu) torch's ASGD stores at the end of the 1-based ``step``, for the next step to use"""
    step = float(step)
    return _f32(lr / ((1 + lambd * lr * step) ** alpha)), _f32(1 / max(1, step - t0))


class _Fused(torch.optim.Optimizer):
    _state_names = ()            # state arrays parallel to the trainable arena
    _scalars = ()                # per-parameter 0-d fp32 state, one value for every parameter, kept on the host
    _stateless = False           # torch keeps no state at all (SGD without momentum): no `step` either
    _eager = False               # torch creates the state of EVERY parameter at construction (Adagrad)
    _fixed = {}                  # param_group settings the kernel does not implement -> the one value it accepts
    _kind = None                 # ops.OPTIM_KINDS entry of the rules that have a device-scalar (capturable) step
    capture_safe = False

    def __init__(self, net, lr, defaults, capturable=False):
        net._ensure_device()
        self.net = net
        self._capturable = bool(capturable)
        if self._capturable:
            if self._kind is None:
                raise ValueError(f"a2c_amd: {type(self).__name__} has no capturable mode")
            defaults = dict(defaults, capturable=True)
            self.capture_safe = True     # no step-dependent kernel argument: [advance, step] replays exactly
        super().__init__(list(net.parameters()), dict(lr=lr, **defaults))
        ar = net._arena
        self._flat = {k: torch.zeros(ar.n_train, dtype=torch.float32, device=ar.params.device)
                      for k in self._state_names}
        self._stats = torch.zeros(2, dtype=torch.float64, device=ar.params.device)   # [sum g^2, -]
        self._scratch = None         # this optimiser's own reduction scratch (ops.new_reduce_scratch), made on first use
        self._norm = torch.zeros(1, dtype=torch.float32, device=ar.params.device)
        self._steps = 0
        self._scal = {}              # host values of self._scalars (set by the first step, or loaded)
        self._name_of = {id(p): n for n, p in net.named_parameters()}
        self._block = ops.optim_block_new(ar.params.device) if self._capturable else None
        if self._eager:
            self._publish_state()

    def _views(self, p):
        o, k, shp = self.net._arena.offsets[self._name_of[id(p)]]
        return {s: self._flat[s][o:o + k].view(shp) for s in self._state_names}

    def _trainable(self, p):
        return self._name_of[id(p)] in self.net._arena.trainable

    def _publish_state(self):
        """Expose the flat state as torch-style per-parameter entries (lazily, like torch, unless _eager)."""
        if self._stateless:
            return
        blk = ops.optim_block_read(self._block) if self._capturable else None     # the device's count, one read-back
        dev = self.net._arena.params.device
        for p in self.param_groups[0]["params"]:
            if not self._trainable(p):
                if self._eager and "step" not in self.state[p]:    # never gets a gradient: torch's initial state
                    self.state[p].update(step=torch.tensor(0.0, dtype=torch.float32),
                                         **{s: torch.zeros_like(p) for s in self._state_names})
                continue
            st = self.state[p]
            if "step" not in st:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st.update(self._views(p))
            if blk is not None:            # torch's capturable layout: 0-d fp32 tensors on the parameter's device
                st["step"] = torch.tensor(float(blk["step"]), dtype=torch.float32, device=dev)
                for k in self._scalars:
                    st[k] = torch.tensor(blk[k], dtype=torch.float32, device=dev)
                continue
            st["step"].fill_(float(self._steps))
            for k in self._scalars:
                st[k] = torch.tensor(self._scal[k], dtype=torch.float32)

    def state_dict(self):
        if self._steps > 0 or self._eager:
            self._publish_state()
        return super().state_dict()

    def _check_group(self, group):
        for k, want in self._fixed.items():
            if k in group and group[k] != want:
                raise ValueError(f"a2c_amd: {type(self).__name__} implements {k}={want!r} only, got {group[k]!r}")
        if self._kind is not None and bool(group.get("capturable", False)) != self._capturable:
            raise ValueError(f"a2c_amd: this {type(self).__name__} was built with capturable={self._capturable!r}; the "
                             "mode is fixed at construction (build a new optimiser and load this one's state_dict)")

    def load_state_dict(self, state_dict):
        if self._kind is not None:
            # a checkpoint written in the other mode (or by torch / the reference) carries ITS `capturable`: the state
            # loads either way and the group keeps this object's mode
            state_dict = dict(state_dict, param_groups=[dict(g, capturable=self._capturable)
                                                        for g in state_dict["param_groups"]])
        for g in state_dict["param_groups"]:
            self._check_group(g)
        super().load_state_dict(state_dict)
        steps = 0
        for p in self.param_groups[0]["params"]:
            st = self.state.get(p)
            if not st or not self._trainable(p):
                continue
            views = self._views(p)
            for s in self._state_names:
                views[s].copy_(st[s])
                st[s] = views[s]
            steps = max(steps, int(float(st["step"])))
            st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
            for k in self._scalars:
                self._scal[k] = _f32(float(st[k]))
                st[k] = torch.tensor(self._scal[k], dtype=torch.float32)
        self._steps = steps
        if self._capturable and steps > 0:
            ops.optim_block_set(self._block, steps, **self._scal)
            self._publish_state()            # the published step / scalars are device tensors in this mode

    def zero_grad(self, set_to_none=False):
        # gradients live in the arena and are overwritten by every backward pass
        pass

    def grad_norm(self):
        """Pre-clip global gradient norm of the last step (device float tensor)."""
        return self._norm

    def _first_step(self):
        """torch's lazy state initialisation at the first step (besides the zeroed arrays): per-rule"""

    @torch.no_grad()
    def step(self, closure=None, max_norm=None, st=None):
        self._check_group(self.param_groups[0])
        ar = self.net._arena
        st = st if st is not None else ops.stream()
        g = ar.train_grads()
        if self._scratch is None or self._scratch.device != g.device:
            self._scratch = ops.new_reduce_scratch(g.device)
        ops.gradnorm_sq(g, self._stats[:1], st, scratch=self._scratch)
        if self._steps == 0:
            self._first_step()
            if self._capturable:
                ops.optim_block_set(self._block, 0, **self._scal)
        self._steps += 1
        max_norm = float("1e30") if max_norm is None else float(max_norm)
        if self._capturable:
            # the device path, whether or not a capture is in progress: eager and graphed runs are the same launches
            self._advance(st)
            fl = [self._flat[k] for k in self._state_names] + [None]
            ops.clip_step_dev(self._kind, ar.train_params(), g, fl[0], fl[1], self._stats, max_norm, self._block,
                              self._norm, st)
        else:
            self._launch(ar.train_params(), g, max_norm, st)
        self.net.mark_dirty()

    def _advance(self, st):
        """a2c_optim_advance with this rule's hyper-parameters (they are arguments of the launch: a capture fixes them)"""
        grp = self.param_groups[0]
        b1, b2 = grp.get("betas", (0.0, 0.0))
        ops.optim_advance(self._kind, self._block, grp["lr"], b1, b2, grp.get("eps", 0.0), grp.get("weight_decay", 0.0),
                          grp.get("momentum_decay", 0.0), grp.get("lambd", 0.0), grp.get("alpha", 0.0),
                          grp.get("t0", 0.0), st)


class RMSprop(_Fused):
    _state_names = ("square_avg",)
    capture_safe = True          # every argument of the step kernel is step-independent (hipGraph replays are exact)

    def __init__(self, net, lr=1e-2, alpha=0.99, eps=1e-8):
        super().__init__(net, lr, dict(alpha=alpha, eps=eps, weight_decay=0, momentum=0, centered=False,
                                       capturable=False, foreach=None, maximize=False, differentiable=False))

    def _launch(self, p, g, max_norm, st):
        grp = self.param_groups[0]
        ops.clip_rmsprop(p, g, self._flat["square_avg"], self._stats, max_norm, grp["lr"], grp["alpha"], grp["eps"],
                         self._norm, st)


class Adam(_Fused):
    _state_names = ("exp_avg", "exp_avg_sq")
    _kind = ops.OPTIM_KINDS["Adam"]

    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, capturable=False):
        super().__init__(net, lr, dict(betas=betas, eps=eps, weight_decay=0, amsgrad=False, maximize=False,
                                       foreach=None, capturable=False, differentiable=False, fused=None,
                                       decoupled_weight_decay=False), capturable)

    def _launch(self, p, g, max_norm, st):
        grp = self.param_groups[0]
        ops.clip_adam(p, g, self._flat["exp_avg"], self._flat["exp_avg_sq"], self._stats, max_norm, grp["lr"],
                      grp["betas"][0], grp["betas"][1], grp["eps"], self._steps, self._norm, st)


def _torch_defaults(name, lr):
    """the param_group settings of torch.optim.<name>(params, lr=lr): the same keys and default values as torch"""
    d = dict(getattr(torch.optim, name)([torch.zeros(1, requires_grad=True)], lr=lr).defaults)
    del d["lr"]
    return d


_NO_DECAY = dict(weight_decay=0, maximize=False)


class SGD(_Fused):
    _stateless = True
    _fixed = dict(momentum=0, dampening=0, nesterov=False, **_NO_DECAY)
    capture_safe = True

    def __init__(self, net, lr=1e-3):
        super().__init__(net, lr, _torch_defaults("SGD", lr))

    def _launch(self, p, g, max_norm, st):
        ops.clip_sgd(p, g, self._stats, max_norm, self.param_groups[0]["lr"], self._norm, st)


class Adagrad(_Fused):
    _state_names = ("sum",)
    _eager = True
    _fixed = dict(initial_accumulator_value=0, **_NO_DECAY)

    def __init__(self, net, lr=1e-2):
        super().__init__(net, lr, _torch_defaults("Adagrad", lr))

    @property
    def capture_safe(self):      # clr = lr / (1 + (step-1) lr_decay) is a kernel argument unless lr_decay == 0
        return self.param_groups[0]["lr_decay"] == 0

    def _launch(self, p, g, max_norm, st):
        grp = self.param_groups[0]
        ops.clip_adagrad(p, g, self._flat["sum"], self._stats, max_norm, grp["lr"], grp["lr_decay"], grp["eps"],
                         self._steps, self._norm, st)


class Adadelta(_Fused):
    _state_names = ("square_avg", "acc_delta")
    _fixed = _NO_DECAY
    capture_safe = True

    def __init__(self, net, lr=1.0):
        super().__init__(net, lr, _torch_defaults("Adadelta", lr))

    def _launch(self, p, g, max_norm, st):
        grp = self.param_groups[0]
        ops.clip_adadelta(p, g, self._flat["square_avg"], self._flat["acc_delta"], self._stats, max_norm, grp["lr"],
                          grp["rho"], grp["eps"], self._norm, st)


class Rprop(_Fused):
    _state_names = ("prev", "step_size")
    _fixed = dict(maximize=False)
    capture_safe = True          # step_size is filled with lr by the first (eager) step, not by the kernel

    def __init__(self, net, lr=1e-2):
        super().__init__(net, lr, _torch_defaults("Rprop", lr))

    def _first_step(self):
        self._flat["step_size"].fill_(self.param_groups[0]["lr"])      # torch.full_like(grad, lr)

    def _launch(self, p, g, max_norm, st):
        grp = self.param_groups[0]
        ops.clip_rprop(p, g, self._flat["prev"], self._flat["step_size"], self._stats, max_norm, grp["etas"][0],
                       grp["etas"][1], grp["step_sizes"][0], grp["step_sizes"][1], self._norm, st)


class AdamW(_Fused):
    _kind = ops.OPTIM_KINDS["AdamW"]
    _state_names = ("exp_avg", "exp_avg_sq")
    _fixed = dict(amsgrad=False, maximize=False, decoupled_weight_decay=True)

    def __init__(self, net, lr=1e-3, capturable=False):
        super().__init__(net, lr, _torch_defaults("AdamW", lr), capturable)

    def _launch(self, p, g, max_norm, st):
        grp = self.param_groups[0]
        ops.clip_adamw(p, g, self._flat["exp_avg"], self._flat["exp_avg_sq"], self._stats, max_norm, grp["lr"],
                       grp["betas"][0], grp["betas"][1], grp["eps"], grp["weight_decay"], self._steps, self._norm, st)


class Adamax(_Fused):
    _kind = ops.OPTIM_KINDS["Adamax"]
    _state_names = ("exp_avg", "exp_inf")
    _fixed = _NO_DECAY

    def __init__(self, net, lr=2e-3, capturable=False):
        super().__init__(net, lr, _torch_defaults("Adamax", lr), capturable)

    def _launch(self, p, g, max_norm, st):
        grp = self.param_groups[0]
        ops.clip_adamax(p, g, self._flat["exp_avg"], self._flat["exp_inf"], self._stats, max_norm, grp["lr"],
                        grp["betas"][0], grp["betas"][1], grp["eps"], self._steps, self._norm, st)


class NAdam(_Fused):
    _kind = ops.OPTIM_KINDS["NAdam"]
    _state_names = ("exp_avg", "exp_avg_sq")
    _scalars = ("mu_product",)
    _fixed = dict(decoupled_weight_decay=False, **_NO_DECAY)

    def __init__(self, net, lr=2e-3, capturable=False):
        super().__init__(net, lr, _torch_defaults("NAdam", lr), capturable)

    def _first_step(self):
        self._scal["mu_product"] = 1.0

    def _launch(self, p, g, max_norm, st):
        grp = self.param_groups[0]
        beta1 = grp["betas"][0]
        self._scal["mu_product"] = nadam_mu_product(self._scal["mu_product"], self._steps, beta1, grp["momentum_decay"])
        ops.clip_nadam(p, g, self._flat["exp_avg"], self._flat["exp_avg_sq"], self._stats, max_norm, grp["lr"], beta1,
                       grp["betas"][1], grp["eps"], grp["momentum_decay"], self._steps, self._scal["mu_product"],
                       self._norm, st)


class RAdam(_Fused):
    _kind = ops.OPTIM_KINDS["RAdam"]
    _state_names = ("exp_avg", "exp_avg_sq")
    _fixed = dict(decoupled_weight_decay=False, **_NO_DECAY)

    def __init__(self, net, lr=1e-3, capturable=False):
        super().__init__(net, lr, _torch_defaults("RAdam", lr), capturable)

    def _launch(self, p, g, max_norm, st):
        grp = self.param_groups[0]
        ops.clip_radam(p, g, self._flat["exp_avg"], self._flat["exp_avg_sq"], self._stats, max_norm, grp["lr"],
                       grp["betas"][0], grp["betas"][1], grp["eps"], self._steps, self._norm, st)


class ASGD(_Fused):
    _kind = ops.OPTIM_KINDS["ASGD"]
    _state_names = ("ax",)
    _scalars = ("eta", "mu")
    _fixed = _NO_DECAY

    def __init__(self, net, lr=1e-2, capturable=False):
        super().__init__(net, lr, _torch_defaults("ASGD", lr), capturable)

    def _first_step(self):
        self._scal.update(eta=_f32(self.param_groups[0]["lr"]), mu=1.0)

    def _launch(self, p, g, max_norm, st):
        grp = self.param_groups[0]
        # this step uses the eta / mu the previous one stored, then stores the next ones (fp32 0-d tensors in torch)
        ops.clip_asgd(p, g, self._flat["ax"], self._stats, max_norm, grp["lambd"], self._scal["eta"], self._scal["mu"],
                      self._norm, st)
        self._scal["eta"], self._scal["mu"] = asgd_eta_mu(self._steps, grp["lr"], grp["lambd"], grp["alpha"], grp["t0"])


# Updater.new_optim's registry: hyps["optim_type"] -> class.  The reference builds any torch.optim class by name;
# the ones missing here cannot run on the reference's nets either, or do not map onto the flat arena.
OPTIMIZERS = {c.__name__: c for c in (RMSprop, Adam, SGD, Adagrad, Adadelta, Rprop, AdamW, Adamax, NAdam, RAdam, ASGD)}
UNSUPPORTED = {
    "LBFGS": "its step() needs a closure",
    "SparseAdam": "it takes sparse gradients only",
    "Muon": "it takes 2-D parameters only",
    "Adafactor": "its factored row / column state does not map onto the flat parameter arena",
}


def check_name(name):
    """ValueError unless ``name`` is in OPTIMIZERS (no device work)"""
    if name not in OPTIMIZERS:
        why = f" ({UNSUPPORTED[name]})" if name in UNSUPPORTED else ""
        raise ValueError(f"a2c_amd: optim_type {name!r} is not supported{why}; supported: {', '.join(OPTIMIZERS)}")
    return OPTIMIZERS[name]
