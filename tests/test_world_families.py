"""The Python around the six device worlds, on the CPU: which library entry point a pool calls with which arguments (the
functions of ``ops`` replaced by recorders), the family records against their modules, the order of ``train()``'s refusals,
and that no list of family names is typed out by hand."""
import ast
import inspect
import os
import re

import pytest
import torch

from a2c_amd import breakout, cartpole, ops, pendulum, point, pong, snake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-a2c_amd", "a2c_amd")
N, SEED, ID0, PTR, STRIDE = 3, 5, 7, 4096, 2
POST, TRUNC = object(), object()


# ---------------------------------------------------------------- 1. which entry point, which arguments
class R:
    """the fields of the ``world_rules`` block an entry point was handed"""

    def __init__(self, *fields):
        self.fields = fields


# tokens: a string names a tensor of the pool (sliced to the env range unless it starts with "ep") or the step's own value
# ("B", "id0": the first env id of the range); everything else is the scalar itself, compared by value and type
HEAD_I, HEAD_F = ("state", PTR, STRIDE, 0, "B", "id0", SEED), ("state", PTR, STRIDE, 0.0, "B", "id0", SEED)
OUT, EP = ("rew", "done", "reset"), ("ep0", "ep1")
PONG_W, BREAKOUT_W, SNAKE_W, POINT_W, CARTPOLE_W, PENDULUM_W = (2, 50, 1, 2), (2, 60), (4, 1, 1), (2, 40), (30,), (20,)
PONG_KW = dict(points_to_win=2, max_episode_steps=50, opp_skill_num=1, opp_skill_den=2)
BREAKOUT_KW = dict(lives=2, max_episode_steps=60)
ONE_FRAME = R(1, 1, 0, 1, 0, 0)


def _register(what, head, world, hw, configs):
    """the rows of a register world (Pong, Breakout): {config: (kwargs, reset row, step row, post row)}"""
    rows = {}
    for cfg, kw, step, step_extra, post, post_extra in configs:
        rows[cfg] = (kw, (what + "_reset", ("STATE", N, ID0, SEED) + world + ("FRAMES", hw)),
                     (what + "_" + step, head + world + ("frames", hw) + OUT + step_extra + EP),
                     (what + "_" + post, head + world + (None, hw) + OUT + post_extra + EP))
    return rows


def _lane(what, head, world, hw):
    """the rows of a lane world: without and with a ``trunc`` block"""
    reset = (what + "_reset", ("STATE", N, ID0, SEED) + world + ("FRAMES", hw))
    return {"plain": ({}, reset, (what + "_step", head + world + ("frames", hw) + OUT + (ONE_FRAME, None) + EP),
                      (what + "_step", head + world + (None, hw) + OUT + (ONE_FRAME, POST) + EP)),
            "trunc": ({}, reset, (what + "_step_trunc", head + world + ("frames", hw) + OUT + (TRUNC, ONE_FRAME, None) + EP),
                      (what + "_step_trunc", head + world + (None, hw) + OUT + (TRUNC, ONE_FRAME, POST) + EP))}


def _register_configs(flags):
    cfgs = [("(1, 0, 1)", dict(frame_skip=1, sticky_num=0, sticky_den=1), "step", (), "step_post", (POST,)),
            ("(4, 1, 4)", dict(frame_skip=4, sticky_num=1, sticky_den=4), "step_skip", (4, 1, 4), "step_post_skip", (4, 1, 4, POST)),
            ("frame_skip_max=6", dict(frame_skip_max=6), "step_rules", (R(1, 6, 0, 1, 0, 0), None), "step_rules",
             (R(1, 6, 0, 1, 0, 0), POST))]
    if flags:
        cfgs.append(("episodic_life", dict(episodic_life=True), "step_rules", (R(1, 1, 0, 1, 1, 0), None), "step_rules",
                     (R(1, 1, 0, 1, 1, 0), POST)))
    return cfgs


SNAKE_RESET = ("snake_reset", ("STATE", N, ID0, SEED) + SNAKE_W + ("FRAMES", "RGB"))
TABLE = {
    "Pong": (pong.DevicePongPool, PONG_KW, _register("pong", HEAD_I, PONG_W, 6400, _register_configs(False))),
    "Breakout": (breakout.DeviceBreakoutPool, BREAKOUT_KW, _register("breakout", HEAD_I, BREAKOUT_W, 5760, _register_configs(True))),
    "Snake": (snake.DeviceSnakePool, dict(grid_size=4, unit_size=1, n_foods=1), {
        "prepped": ({}, SNAKE_RESET, ("snake_step", HEAD_I + SNAKE_W + OUT + ("frames", "rgb", "EP_STATS")),
                    ("snake_step_post", HEAD_I + SNAKE_W + OUT + (None, POST, "rgb", "EP_STATS"))),
        "raw_frames": (dict(raw_frames=True), SNAKE_RESET, ("snake_step", HEAD_I + SNAKE_W + OUT + ("frames", "rgb", "EP_STATS")),
                       ("snake_step_post", HEAD_I + SNAKE_W + OUT + (None, POST, "rgb", "EP_STATS")))}),
    "Point": (point.DevicePointPool, dict(targets_to_win=2, max_episode_steps=40), _lane("point", HEAD_F, POINT_W, 8)),
    "CartPole": (cartpole.DeviceCartPolePool, dict(max_episode_steps=30), _lane("cartpole", HEAD_I, CARTPOLE_W, 4)),
    "Pendulum": (pendulum.DevicePendulumPool, dict(max_episode_steps=20), _lane("pendulum", HEAD_F, PENDULUM_W, 4)),
}
CASES = [(fam, cfg) for fam, (_, _, rows) in TABLE.items() for cfg in rows]


@pytest.fixture
def calls(monkeypatch):
    """every world reset / step function of ``ops`` replaced by a recorder: [(name, positional arguments)]"""
    log = []
    names = [n for n in dir(ops) if re.fullmatch(r"(pong|breakout|snake|point|cartpole|pendulum)_(reset|step\w*)", n)]
    assert len(names) == 6 + 2 + 5 + 5 + 3 * 2
    for n in names:
        def rec(*a, _n=n, **k):
            assert not k, (_n, k)
            log.append((_n, a))
        monkeypatch.setattr(ops, n, rec)
    return log


def _same(got, want, pool, env0, B):
    sl = slice(env0, env0 + B)
    tensors = {"state": pool.state[sl], "frames": pool.frames[sl], "rew": pool.rew[sl], "done": pool.done[sl],
               "reset": pool.reset_mask[sl], "ep0": pool.ep_stats[0:1], "ep1": pool.ep_stats[1:2], "EP_STATS": pool.ep_stats,
               "STATE": pool.state, "FRAMES": pool.frames}
    rgb = getattr(pool, "rgb", None)
    tensors.update(RGB=rgb, rgb=None if rgb is None else rgb[sl])
    if isinstance(want, str) and want in ("B", "id0"):
        want = B if want == "B" else ID0 + env0
    if isinstance(want, str):
        t = tensors[want]
        if t is None:
            return got is None
        return isinstance(got, torch.Tensor) and got.data_ptr() == t.data_ptr() and got.shape == t.shape and got.dtype == t.dtype
    if isinstance(want, R):
        return got is pool.rules and tuple(getattr(got, f) for f in ("frame_skip", "frame_skip_max", "sticky_num", "sticky_den",
                                                                     "episodic_life", "clip_rewards")) == want.fields
    if want is None or want is POST or want is TRUNC:
        return got is want
    return type(got) is type(want) and got == want


def _check(call, row, pool, env0, B):
    assert call[0] == row[0]
    assert len(call[1]) == len(row[1]), (call[0], len(call[1]), len(row[1]))
    for i, (g, w) in enumerate(zip(call[1], row[1])):
        assert _same(g, w, pool, env0, B), (call[0], i, g, w)


@pytest.mark.parametrize("fam,cfg", CASES)
def test_pool_calls_the_entry_point_with_the_arguments(fam, cfg, calls):
    cls, world, rows = TABLE[fam]
    kw, reset_row, step_row, post_row = rows[cfg]
    pool = cls(N, "cpu", seed=SEED, env_id0=ID0, **world, **kw)
    trunc = TRUNC if cfg == "trunc" else None
    assert type(pool.action_shift) is type(step_row[1][3]) and pool.action_shift == 0
    pool.reset_all()
    out = pool.step(PTR, STRIDE, trunc=trunc)
    assert out[0].data_ptr() == pool.frames.data_ptr() and out[0].shape == pool.frames.shape
    pool.step(PTR, STRIDE, 1, 2, trunc=trunc)
    out = pool.device_step_post(0, 0, N, (PTR, STRIDE), POST, trunc=trunc)
    assert [o.data_ptr() for o in out] == [pool.rew.data_ptr(), pool.done.data_ptr(), pool.reset_mask.data_ptr()]
    pool.device_step_post(3, 1, 2, (PTR, STRIDE), POST, trunc=trunc)
    assert len(calls) == 5
    _check(calls[0], reset_row, pool, 0, N)
    _check(calls[1], step_row, pool, 0, N)
    _check(calls[2], step_row, pool, 1, 2)
    _check(calls[3], post_row, pool, 0, N)
    _check(calls[4], post_row, pool, 1, 2)


def test_register_pools_share_one_base():
    from a2c_amd import worlds
    for cls, what in ((pong.DevicePongPool, "Pong"), (breakout.DeviceBreakoutPool, "Breakout")):
        assert issubclass(cls, worlds.DeviceRegisterWorldPool) and cls.WHAT == what
        assert "_step" not in vars(cls) and "_reset" not in vars(cls)
    assert not issubclass(snake.DeviceSnakePool, worlds.DeviceRegisterWorldPool)
    p = pong.DevicePongPool(N, "cpu", frame_skip=2)
    assert (p.world, p.repeat, p.rules, p.plain, p.frame_shape) == ((21, 10000, 3, 4), (2, 0, 1), None, False, (1, 80, 80))
    b = breakout.DeviceBreakoutPool(N, "cpu", clip_rewards=True)
    assert (b.world, b.repeat, b.plain, b.frame_shape) == ((5, 10000), (1, 0, 1), False, (1, 80, 72)) and b.rules.clip_rewards == 1
    assert breakout.DeviceBreakoutPool(N, "cpu").plain and pong.DevicePongPool(N, "cpu").plain


# ---------------------------------------------------------------- 2. the registry against the modules
MODULES = {"Snake": snake, "Pong": pong, "Breakout": breakout, "Point": point, "CartPole": cartpole, "Pendulum": pendulum}
# (preprocessor, the "Pong" done override, one-bit frames, frame_skip / sticky_* taken, models)
STATED = {"Snake": ("snake_prep", False, False, False, None), "Pong": ("pong_prep", True, True, True, None),
          "Breakout": ("breakout_prep", False, False, True, None),
          "Point": ("null_prep", False, False, True, ("FCModel", "GRUFCModel")),
          "CartPole": ("null_prep", False, False, True, ("FCModel", "GRUFCModel")),
          "Pendulum": ("null_prep", False, False, True, ("FCModel", "GRUFCModel"))}
RULES = {"Snake": (), "Pong": ("frame_skip_max",), "Breakout": ("frame_skip_max", "episodic_life", "clip_rewards"),
         "Point": ("frame_skip_max",), "CartPole": ("frame_skip_max",), "Pendulum": ("frame_skip_max",)}


def _declared(fn, keys):
    p = inspect.signature(fn).parameters
    return tuple(p[k].default for k in keys)


@pytest.mark.parametrize("name", list(MODULES))
def test_family_record_agrees_with_its_module(name, monkeypatch):
    from a2c_amd import families, preprocessing
    mod = MODULES[name]
    fam = mod.FAMILY
    # twin, pool and factory are the module's, also where someone rebinds them there (a test's recording subclass)
    with monkeypatch.context() as m:
        sub = type("Recording", (fam.pool,), {})
        m.setattr(mod, "Device" + name + "Pool", sub)
        m.setattr(mod, name + "Factory", ast.literal_eval)
        assert fam.pool is sub and fam.factory is ast.literal_eval
    assert families.FAMILIES[name] is fam and list(families.FAMILIES) == list(MODULES)
    env, pool = getattr(mod, name + "Env"), getattr(mod, "Device" + name + "Pool")
    assert (fam.name, fam.env, fam.pool, fam.check_world) == (name, env, pool, mod.check_world)
    assert (fam.prep, fam.pong_done, fam.frame_bits, fam.repeats, fam.models) == STATED[name]
    assert callable(getattr(preprocessing, fam.prep))
    assert fam.device_prep == ("breakout_prep" if name == "Breakout" else None)
    # what the pool class says is read from it
    cont = bool(getattr(pool, "float_actions", False))
    assert fam.float_actions is cont and cont == (name in ("Point", "Pendulum"))
    assert fam.n_act == (mod.ACTION_SIZE if cont else mod.N_ACTIONS) and (pool.n_act == fam.n_act if cont else True)
    assert fam.reports_trunc is pool.reports_trunc
    keys = tuple(k for k, _ in fam.world_keys)
    if name == "Snake":
        assert fam.frame_shape(dict(grid_size=6, unit_size=2)) == (1, 12, 12) and not fam.vector
    else:
        assert fam.frame_shape(dict.fromkeys(keys)) == pool.frame_shape and fam.vector == (len(pool.frame_shape) == 2)
    # the defaults, against the constructors of the twin and of the pool
    dflt = tuple(d for _, d in fam.world_keys)
    assert dflt == _declared(env.__init__, keys) == _declared(pool.__init__, keys)
    assert fam.world_from_hyps({}) == mod.world_from_hyps({}) == dflt
    assert fam.world_from_hyps(dict.fromkeys(keys)) == dflt
    assert mod.world_from_hyps == fam.world_from_hyps and mod.rules_from_hyps == fam.rules_from_hyps if name != "Snake" else True
    assert fam.rule_keys == RULES[name] and (name == "Snake" or mod.RULE_KEYS == fam.rule_keys)
    assert fam.rules_from_hyps({}) == dict(zip(("frame_skip_max", "episodic_life", "clip_rewards"), (1, False, False)[:len(RULES[name])]))
    assert fam.repeat_from_hyps(dict(frame_skip=3, sticky_num=1, sticky_den=4)) == (3, 1, 4)
    e = getattr(mod, name + "Factory")(env_id=4, seed=2)()
    assert type(e) is env and e.env_id == 4 and type(fam.factory(env_id=1)()) is env


def test_name_lists_are_those_that_were_typed_out():
    from a2c_amd import families, training
    assert families.DEVICE_TYPES == ("Snake-device", "Pong-device", "Breakout-device", "Point-device", "CartPole-device",
                                     "Pendulum-device")
    assert families.LANE_DEVICE_TYPES == ("Point-device", "CartPole-device", "Pendulum-device")
    assert families.VECTOR_WORLDS == training._VECTOR_WORLDS == ("Point", "CartPole", "Pendulum")
    assert training._WORLDS is families.FAMILIES and set(training._WORLDS) == set(MODULES)
    for name in MODULES:
        assert training._world_family(name + "-device") == training._world_family(name + "-host") == name
    for other in ("Pong-v0", "Pong", "Pong-gpu", "Reach-device", None):
        assert training._world_family(other) is None


def test_messages_keep_their_names_in_order():
    from a2c_amd import vecnorm
    from a2c_amd.runner import DeviceStatsRunner, check_bootstrap_truncated
    with pytest.raises(ValueError) as e:
        check_bootstrap_truncated(dict(env_type="Pong-device"))
    assert str(e.value) == ("a2c_amd: bootstrap_truncated bootstraps time-limit episode ends of the lane worlds' device pools "
                            "(env_type 'Point-device', 'CartPole-device', 'Pendulum-device'), not 'Pong-device'")
    with pytest.raises(ValueError) as e:
        check_bootstrap_truncated(dict(env_type="Pong-device"), pool=object())
    assert str(e.value) == ("a2c_amd: bootstrap_truncated needs a device env pool whose step reports the state an episode ended "
                            "in (DevicePointPool, DeviceCartPolePool, DevicePendulumPool), not object")
    with pytest.raises(ValueError) as e:
        vecnorm.check_runner(dict(norm_obs=True), object(), None, False, ranks=1)
    assert str(e.value) == ("norm_obs: running normalisation lives in the slot of a DEVICE env pool (Point-device, "
                            "CartPole-device, Pendulum-device); this is a host env pool")
    with pytest.raises(ValueError) as e:
        DeviceStatsRunner({}, object())
    assert str(e.value) == ("DeviceStatsRunner: a device env pool with device_step_post (Snake / Pong / Breakout / Point / "
                            "CartPole / Pendulum worlds)")


# ---------------------------------------------------------------- 3. the order of train()'s refusals; nothing written
def _factory(j):
    raise AssertionError("train() built an env")


REFUSALS = [
    ("bad gauss_loss before bootstrap_truncated + env_fn",
     dict(env_type="Pendulum-device", gauss_loss="bogus", bootstrap_truncated=True), _factory,
     "a2c_amd: hyps['gauss_loss'] is 'reference' or 'exact', not 'bogus'"),
    ("bad eval_pool before norm_obs on a picture world", dict(env_type="Pong-device", eval_pool="gpu", norm_obs=True), None,
     "a2c_amd: hyps['eval_pool'] is 'host' or 'device', not 'gpu'"),
    ("Snake's frame skip before its frame_skip_max", dict(env_type="Snake-device", frame_skip=2, frame_skip_max=3), None,
     "a2c_amd: frame_skip / sticky_num are keys of the Pong and Breakout worlds: the Snake worlds play one game frame per step"),
    ("a key of another family before the model", dict(env_type="CartPole-device", model="A3CModel", episodic_life=1), None,
     "a2c_amd: episodic_life: not a key of the CartPole worlds (frame_skip_max: Pong and Breakout; episodic_life, clip_rewards: "
     "Breakout)"),
    ("the model before the env pool", dict(env_type="Point-host", env_pool="process", model="ConvModel"), None,
     "a2c_amd: the Point worlds take 2 float actions: model FCModel / GRUFCModel with is_discrete=False, not 'ConvModel'"),
]


@pytest.mark.parametrize("what,kw,env_fn,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_train_refuses_in_order_and_writes_nothing(what, kw, env_fn, text, tmp_path, monkeypatch):
    from a2c_amd.training import train

    def no_device(*a, **k):
        raise AssertionError("train() touched the device")
    monkeypatch.setattr(torch.Tensor, "cuda", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    hyps = dict(dict(exp_name="refusals", main_path=str(tmp_path), model="FCModel", n_envs=2, n_rollouts=2, n_tsteps=2,
                     n_frame_stack=2, max_tsteps=1e9, seed=1, h_size=16), **kw)
    with pytest.raises(ValueError) as e:
        train(None, hyps, verbose=False, max_epochs=1, env_fn=env_fn)
    assert str(e.value) == text
    assert not list(tmp_path.iterdir()), "nothing was written"


# ---------------------------------------------------------------- 4. no hand-typed family lists
@pytest.mark.parametrize("module", ["training.py", "runner.py", "vecnorm.py"])
def test_no_list_of_device_env_types_is_typed_out(module):
    tree = ast.parse(open(os.path.join(PKG, module)).read())
    for node in ast.walk(tree):
        if isinstance(node, (ast.Tuple, ast.List)):
            typed = [e.value for e in node.elts if isinstance(e, ast.Constant) and isinstance(e.value, str)
                     and e.value.endswith("-device")]
            assert len(typed) < 2, (module, node.lineno, typed)
