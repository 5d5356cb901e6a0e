"""GPU tests of the native encoder backward (csrc/occ_encoder_bwd.hpp, occlusionenv_amd/enctrain.py, harness.train_predictor)
against tests/train_model.py (the dense encoder-only ``Net``) in f64 on the CPU, torch autograd supplying the gradients.  The
bodies this module shares with tests/test_gpu_sep_encoder_train.py are in tests/train_gpu_suite.py; FORM below is what they
are given.

Weights: train_model.dense_state_dict rounded to f32 (what a checkpoint on disk holds), used as exactly those
values in f64 by the host model; presets "predictor" (no residual, tanh head) and a dense "ppo"-keyed encoder (dilation 1,
residual).  Inputs: encoder_model.make_obs; the upstream grad_feats is randn.

Shapes: S=32 N=2 (the last down output is 1x1, the deepest layers 2x2: the halo is nearly all padding), S=40 N=3 (sides 40 /
20 / 10 / 5 / 3 / 2: odd and even stride-2 edges, 8- and 16-pixel tiles), S=96 N=2 (several 16-pixel tiles per side).  In all
of these a block of the weight gradient owns one pixel tile.  The split case "ppo" S=32 N=129 gives it 5, 5, 5, 2, 2, 2 tiles
per slice on the first six layers and 2, 3, 3, 5 on the last four, with a short last slice and slices that cross env
boundaries (asserted without a GPU in tests/test_encoder_train_host.py); there the backward also runs with an upstream
gradient in one env alone (the last env, which alone fills the short last slice of the level-0 layers, and env 1, where their
first slice that crosses an env boundary ends), and through the C entry points on guarded buffers of exactly the queried
sizes, again after everything it may only write was filled with NaNs.

Bars.  Kept relu outputs: within 1e-4 max(1, max |r64|) of the f64 relu(u).  Gates r > 0: may differ from the f64 gate only
where |u64| <= 1e-4 max(1, max |u64|).  Gradients: per tensor max |got - want| <= 1e-4 max |want| (no floor), the oracle
evaluated with the GPU's own gates (relu(u) replaced by u * gate), so that a flipped borderline pixel is judged by the gate
test and not smeared into every weight sum.

Measured on an MI355X against the f64 model (worst relative error per tensor kind; the bar is 1e-4):
                     conv.weight  conv.bias  bn.weight  bn.bias  head weight  head bias
  one tile per block   2.1e-6      2.0e-6     3.9e-6    1.5e-6
  through head + MSE   3.3e-6      3.3e-6     3.6e-6    2.7e-6     1.7e-6      4.3e-7
  split case           6.6e-7      4.1e-7     8.9e-7    4.1e-7
  one env alone        1.1e-6      8.5e-7     1.4e-6    7.7e-7
Kept relu outputs: 2.0e-6; no gate differed from the f64 gate in any case.  With `env` taken from the slice's first tile, or
with the tile loop ended after one tile, the gradient test of the split case and both one-env tests fail and every one-tile
case still passes (checked by hand)."""
import numpy as np
import pytest
import torch

from occlusionenv_amd.enctrain import TrainableEncoder
from tests import train_gpu_suite as suite
from tests import train_model as m

pytestmark = pytest.mark.gpu

TOL = 1e-4
SPLIT = m.ENCODER_SPLIT_CASE
CASES = [(p, s, n) for s, n in ((32, 2), (40, 3), (96, 2)) for p in ("predictor", "ppo")] + [SPLIT]
IDS = [f"{p}-S{s}-N{n}" for p, s, n in CASES]
WORST = {}  # measured worst relative error per tensor kind (printed with -s)
FORM = suite.Form(
    net=TrainableEncoder, model=lambda case: m.Net(case[0], False, 1, case[0] == "ppo"),
    symbols=("occ_encoder_train_workspace_query", "occ_encoder_train_forward", "occ_encoder_backward"),
    label=lambda case: "{} S={} N={}".format(*case),
    n_params=64, seed=7000, steps=40, tol=TOL, finite_losses=True)


@pytest.fixture(scope="module")
def nets():
    from occlusionenv_amd.encoder import FrozenEncoder

    out = {}
    for preset in ("predictor", "ppo"):
        sd32 = {k: v.float() for k, v in m.dense_state_dict(preset, 31 if preset == "ppo" else 32).items()}
        kw = dict(dilation=1, residual=True) if preset == "ppo" else {}
        out[preset] = (sd32, FrozenEncoder.from_state_dict(sd32, preset=preset, **kw))
    return out


@pytest.fixture(scope="module")
def runs(nets):
    """Per case, computed once and left unchanged: one native forward + backward with a seeded randn upstream gradient, the
    kept relu outputs, and the host model."""
    return suite.make_runs(FORM, nets)


@pytest.mark.parametrize("preset,img,n", CASES, ids=IDS)
def test_forward_identity(runs, preset, img, n):
    suite.forward_identity(FORM, runs(preset, img, n), (preset, img, n))


@pytest.mark.parametrize("preset,img,n", CASES, ids=IDS)
def test_kept_relu_and_gate(runs, preset, img, n):
    suite.kept_relu_and_gates(FORM, runs(preset, img, n), (preset, img, n))


@pytest.mark.parametrize("preset,img,n", CASES, ids=IDS)
def test_gradients_against_f64_autograd(runs, preset, img, n):
    suite.gradients_against_f64_autograd(FORM, WORST, runs(preset, img, n), (preset, img, n))


@pytest.mark.parametrize("preset,img,n", CASES[:6], ids=IDS[:6])
def test_gradients_through_the_head_and_mse(runs, preset, img, n):
    suite.gradients_through_the_head_and_mse(FORM, WORST, runs(preset, img, n), (preset, img, n))


@pytest.mark.parametrize("env", [SPLIT[2] - 1, 1])
def test_gradients_of_one_env(runs, env):
    """The upstream gradient is randn in one env and zero in the others, so that env's tiles are the whole signal."""
    suite.gradients_of_one_env(FORM, WORST, runs(*SPLIT), SPLIT, env)


def test_reproducible_and_accumulating(runs):
    suite.reproducible_and_accumulating(runs("ppo", 40, 3))


@pytest.mark.parametrize("preset,img,n", [SPLIT, ("predictor", 40, 3)], ids=[IDS[6], IDS[2]])
def test_no_stale_reads_and_nothing_outside_the_reported_sizes(runs, preset, img, n):
    """The native calls on guarded buffers of exactly the queried sizes, and the backward again after everything it may only
    write has been filled with NaNs (suite.no_stale_reads_and_nothing_outside_the_reported_sizes)."""
    suite.no_stale_reads_and_nothing_outside_the_reported_sizes(FORM, runs(preset, img, n), (preset, img, n))


@pytest.fixture(scope="module")
def trained(runs):
    """Forty AdamW steps at lr 1e-3 on a fixed batch ("predictor", S=40, N=3) towards fixed unit targets."""
    return suite.trained_encoder(FORM, runs("predictor", 40, 3))


def test_learning(trained):
    print("native MSE:", trained["losses"][0], "->", trained["losses"][-1])
    suite.learning(FORM, trained)


def test_round_trip_into_a_frozen_encoder(trained):
    net, enc, obs = trained["net"], trained["enc"], trained["obs"]
    sd = net.state_dict()
    assert "features.initial.conv.weight" in sd and "features.features.4.down.bn.running_var" in sd and "output.bias" in sd
    assert tuple(sd["features.features.4.down.conv.weight"].shape) == (256, 128, 3, 3)
    tuned = enc.with_encoder(sd)
    with torch.no_grad():
        now = net(obs)
        grad_now = net.predict_grad(obs)
    assert torch.equal(tuned(obs), now)
    assert not torch.equal(now, trained["feats0"])
    assert torch.equal(enc(obs), trained["feats0"])  # the untouched encoder keeps its feature
    assert torch.allclose(tuned.predict_grad(obs), grad_now, rtol=1e-5, atol=1e-6)  # addmm against F.linear


def test_errors(nets, runs):
    from occlusionenv_amd.encoder import FrozenEncoder
    from tests.encoder_model import golden_state_dict
    import os

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_golden.npz"))
    sep = FrozenEncoder.from_state_dict({k: v.float() for k, v in golden_state_dict(g, "ppo").items()}, preset="ppo")
    assert sep.separable
    with pytest.raises(ValueError, match="separable"):
        TrainableEncoder.from_encoder(sep)
    sd32 = nets["predictor"][0]
    with pytest.raises(ValueError, match="dilation 1"):
        TrainableEncoder.from_encoder(FrozenEncoder.from_state_dict(sd32, preset="predictor", dilation=2))
    suite.errors_tail(FORM, runs("predictor", 40, 3))


def test_train_predictor_harness(nets):
    from environment import OcclusionEnv
    from occlusionenv_amd import environment, harness
    from occlusionenv_amd.meshes import SyntheticShapeNet
    from SubProcVecEnv import SimpleVecEnv

    ds = SyntheticShapeNet(n_models=8, seed=1234)
    environment.seed_scene_rng(78)
    np.random.seed(78)
    torch.manual_seed(78)
    venv = SimpleVecEnv([lambda: OcclusionEnv(ds, img_size=64) for _ in range(4)])
    net = TrainableEncoder.from_encoder(nets["predictor"][1])
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    res = harness.train_predictor(venv, net, 4)
    assert res["net"] is net and res["steps"] + res["skipped"] == 4 and res["steps"] >= 1
    assert len(res["losses"]) == res["steps"] and all(np.isfinite(v) for v in res["losses"])
    assert all(not torch.equal(v, before[k]) for k, v in net.named_parameters())
    res = harness.train_predictor(venv, nets["predictor"][1], 1)  # from an encoder: a net is made
    assert isinstance(res["net"], TrainableEncoder)
