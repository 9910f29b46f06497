"""Continuous (Gaussian) action spaces on FCModel / GRUFCModel: the host-side surface (no GPU needed).  The numbers are
checked on the GPU in test_gpu_continuous.py against tests/golden/g10_continuous.npz (recorded from the reference)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import a2c_amd
from a2c_amd.runner import SequentialEnvironment
from a2c_amd.updater import Updater
import cont_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference/a2c"


@pytest.mark.parametrize("kind", ["FCModel", "GRUFCModel"])
@pytest.mark.parametrize("n", [1, 2, 6])
def test_continuous_models_construct_with_reference_layout(kind, n):
    net = getattr(a2c_amd, kind)(list(CC.STATE_SHAPE), n, h_size=16, is_discrete=False)
    assert net.is_discrete is False
    sd = net.state_dict()
    ref = CC.state_dict(kind, n, 16)
    assert list(sd) == list(ref)
    for k in sd:
        assert tuple(sd[k].shape) == tuple(ref[k].shape), k
    assert tuple(sd["action_out.weight"].shape) == (2 * n, 16) and tuple(sd["action_out.bias"].shape) == (2 * n,)
    net.load_state_dict(ref)            # a reference-layout checkpoint loads
    assert torch.equal(net.state_dict()["action_out.bias"], ref["action_out.bias"])


def test_state_dict_shapes_match_the_recorded_reference(golden):
    g = golden["g10_continuous"]
    for i, (kind, n, h, _B) in enumerate(CC.MODEL_CASES):
        net = getattr(a2c_amd, kind)(list(CC.STATE_SHAPE), n, h_size=h, is_discrete=False)
        mine = [f"{k}:{tuple(t.shape)}" for k, t in net.state_dict().items()]
        assert sorted(mine) == sorted(str(s) for s in g[f"fwd{i}_shapes"]), (kind, n)


def test_discrete_models_unchanged_and_other_models_still_refuse():
    net = a2c_amd.FCModel([1, 1, 5], 3, h_size=16)
    assert net.is_discrete and tuple(net.action_out.weight.shape) == (3, 16)
    for cls, shape in ((a2c_amd.A3CModel, [4, 84, 84]), (a2c_amd.ConvModel, [4, 84, 84]), (a2c_amd.GRUModel, [4, 84, 84])):
        with pytest.raises(NotImplementedError, match="FCModel and GRUFCModel"):
            cls(shape, 3, is_discrete=False)
    for cls in (a2c_amd.FCModel, a2c_amd.GRUFCModel):
        with pytest.raises(NotImplementedError):
            cls([1, 1, 5], 2, bnorm=True)


def test_sequential_environment_box_space_and_gaussian_get_action():
    env = SequentialEnvironment("ContEnv", lambda o: o[None], env_fn=lambda: CC.ContEnv(3))
    assert env.is_discrete is False and env.n == 3
    mu, sigma = torch.tensor([[0.5, -1.0, 2.0]]), torch.tensor([[0.1, 2.0, 1e-4]])
    noise = torch.tensor([[1.0, -0.5, 3.0]])
    a = env.get_action((mu, sigma), noise=noise)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (3,)
    np.testing.assert_array_equal(a, (mu + sigma * noise).numpy()[0])
    a = env.get_action((mu, sigma))                     # default noise: torch.randn_like
    assert a.shape == (3,) and np.all(np.isfinite(a))
    env1 = SequentialEnvironment("ContEnv", lambda o: o[None], env_fn=lambda: CC.ContEnv(1))
    a1 = env1.get_action((torch.tensor([[0.25]]), torch.tensor([[1.0]])), noise=torch.tensor([[2.0]]))
    assert a1.shape == (1,) and a1[0] == np.float32(2.25)


def test_updater_accepts_continuous_nets():
    net = a2c_amd.FCModel(list(CC.STATE_SHAPE), 2, h_size=16, is_discrete=False)
    if torch.cuda.is_available():
        assert Updater(net, CC.cont_hyps()).is_discrete is False
    else:       # past the action-space checks, the optimiser needs the device
        with pytest.raises(RuntimeError, match="HIP device"):
            Updater(net, CC.cont_hyps())
    with pytest.raises(ValueError):
        Updater(net, CC.cont_hyps(is_discrete=True))


def test_train_refuses_the_process_pool_for_continuous_envs(tmp_path):
    from a2c_amd.training import train
    hyps = dict(exp_name="c", main_path=str(tmp_path), model="FCModel", env_type="ContEnv", n_envs=2, n_rollouts=2,
                n_tsteps=3, max_tsteps=1e9, action_size=2, is_discrete=False, env_pool="process", seed=1)
    with pytest.raises(ValueError, match="serial"):
        train(None, hyps, verbose=False, env_fn=lambda j: CC.ContEnv(2, env_id=j, prepped=True), max_epochs=1)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is only in the build container")
def test_g10_regenerates_bit_identically(tmp_path):
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import make_golden_continuous as M; "
            "np.savez(%r, **M.build())" % (os.path.join(ROOT, "tests", "golden"), str(tmp_path / "g10.npz")))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=str(tmp_path), capture_output=True)
    new = np.load(tmp_path / "g10.npz")
    old = np.load(os.path.join(ROOT, "tests", "golden", "g10_continuous.npz"))
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
