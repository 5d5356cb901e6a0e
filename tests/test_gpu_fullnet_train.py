"""GPU tests of the native joint backward (csrc/occ_fullnet_bwd.hpp, occlusionenv_amd/fullnet.py, harness.pretrain_epoch)
against tests/train_model.py (the dense joint ``Net``) in f64 on the CPU with torch autograd.  The bodies this module shares
with tests/test_gpu_sep_fullnet_train.py are in tests/train_gpu_suite.py; FORM below is what they are given.

Weights: train_model.state_dict rounded to f32 (what a checkpoint on disk holds), used as exactly those values in
f64 by the host model.  Inputs: encoder_model.make_obs.  Upstream: a randn grad_feats and a randn grad_prob together.

Shapes: S=32 N=2 (the deepest decoder plane is 1 x 1: the new input gradient of the deepest level), S=64 N=3, S=96 N=2 (sides
96 / 48 / 24 / 12 / 6 / 3), presets "ppo" and "segmenter", residual 1 and 0.  Split cases: "ppo" 129 x 32^2 (the encoder's)
and "ppo" 65 x 96^2 (the decoder's), where the dW slices span several tiles and cross env boundaries on both sides
(asserted below from the two split models), also with both upstream gradients non-zero in one env alone.

Bar: per tensor max |got - want| <= 1e-4 max |want| (no floor), the oracle evaluated with the GPU's own 21 gates
(relu(u) replaced by u * gate), as in the encoder's and the decoder's tests.

Every gradient test prints its relative errors and the worst so far per parameter kind (``-s``); DESIGN.md section 4.4,
"Joint training", is where measured figures are recorded."""
import pytest
import torch

from occlusionenv_amd.enctrain import TrainableEncoder
from occlusionenv_amd.fullnet import TrainableFullNetwork
from tests import decoder_split_model as dsm
from tests import train_gpu_suite as suite
from tests import train_layout as tl
from tests import train_model as m

pytestmark = pytest.mark.gpu

TOL = 1e-4
CASES = m.JOINT_GRAD_CASES + m.JOINT_SPLIT_CASES
IDS = [f"{p}-res{r}-S{s}-N{n}" for p, r, s, n in CASES]
WORST = {}  # measured worst relative error per parameter kind (printed with -s)
FORM = suite.Form(
    net=TrainableFullNetwork, model=lambda case: m.Net(case[0], False, 1, bool(case[1]), True), encoder_net=TrainableEncoder,
    symbols=("occ_fullnet_train_workspace_query", "occ_fullnet_train_forward", "occ_fullnet_backward"),
    label=lambda case: "{} res{} S={} N={}".format(*case), n_params=64 + 22, seed=9000, steps=40, tol=TOL)


@pytest.fixture(scope="module")
def nets():
    from occlusionenv_amd.encoder import FrozenEncoder

    out = {}
    for preset in m.JOINT_PRESETS:
        sd32 = {k: v.float() for k, v in m.state_dict(preset).items()}
        for residual in (1, 0):
            out[preset, residual] = (sd32, FrozenEncoder.from_state_dict(sd32, preset=preset, dilation=1, residual=bool(residual)))
    return out


@pytest.fixture(scope="module")
def runs(nets):
    """Per case, computed once and left unchanged: one native forward + backward with seeded randn upstream gradients, the
    gates of the 21 kept relu outputs, and the host model."""
    return suite.make_runs(FORM, nets)


def test_split_cases_reach_the_tile_loops_on_both_sides():
    """What the split cases have to reach, from the two split models alone: at least two tiles per slice in some encoder
    layer and in some decoder level of each, slices that cross env boundaries on both sides, and a short last slice."""
    for _p, _r, img, n in m.JOINT_SPLIT_CASES:
        enc, dec = tl.dw_plans(img, n), dsm.dw_plans(img, n)
        assert max(p["tps"] for p in enc) >= 2 and max(p["tps"] for p in dec) >= 2, (img, n)
        assert any(p["tps"] >= 2 and p["straddles"] for p in enc) and any(p["short_last"] for p in enc)
        # a decoder slice of more tiles than an env has crosses env boundaries whatever its start
        assert any(p["tps"] >= 2 and (p["straddles"] or p["tps"] > p["tiles_env"]) for p in dec)
    assert [p["tps"] for p in tl.dw_plans(32, 129)] == [5, 5, 5, 2, 2, 2, 1, 1, 1, 1, 1, 1, 2, 3, 3, 5]
    assert [p["tps"] for p in dsm.dw_plans(32, 129)] == [3, 1, 1, 1, 2]
    assert [p["tps"] for p in tl.dw_plans(96, 65)] == [19, 19, 19, 5, 5, 5, 2, 2, 2, 2, 3, 3, 3, 5, 5, 3]
    assert [p["tps"] for p in dsm.dw_plans(96, 65)] == [2, 2, 2, 2, 5]
    assert any(p["short_last"] for p in dsm.dw_plans(96, 65)) and sum(p["straddles"] for p in dsm.dw_plans(96, 65)) == 3


@pytest.mark.parametrize("preset,residual,img,n", CASES, ids=IDS)
def test_forward_identity(runs, preset, residual, img, n):
    suite.forward_identity(FORM, runs(preset, residual, img, n), (preset, residual, img, n))


@pytest.mark.parametrize("preset,residual,img,n", CASES, ids=IDS)
def test_gradients_against_f64_autograd(runs, preset, residual, img, n):
    suite.gradients_against_f64_autograd(FORM, WORST, runs(preset, residual, img, n), (preset, residual, img, n))


@pytest.mark.parametrize("losses", ["dice+mse", "bce+smoothl1"])
def test_gradients_through_the_real_losses(runs, losses):
    """pretrainer.py:127-131 on net(obs): the segmentation loss plus the gradient loss on the head, 88 parameters."""
    case = ("ppo", 1, 64, 3)
    suite.gradients_through_the_real_losses(FORM, WORST, runs(*case), case, losses)


@pytest.mark.parametrize("which", ["last", "one"])
@pytest.mark.parametrize("preset,residual,img,n", m.JOINT_SPLIT_CASES, ids=IDS[-2:])
def test_gradients_of_one_env(runs, preset, residual, img, n, which):
    """Both upstream gradients are randn in one env and zero in the others: a tile given to the wrong env or dropped from a
    short last slice is the whole signal."""
    env = n - 1 if which == "last" else 1
    suite.gradients_of_one_env(FORM, WORST, runs(preset, residual, img, n), (preset, residual, img, n), env)


@pytest.mark.parametrize("preset,residual,img,n", [("ppo", 1, 32, 2), ("ppo", 1, 96, 2), ("segmenter", 0, 64, 3)])
def test_the_join_itself(runs, preset, residual, img, n):
    """grad_feats = 0: whatever reaches the encoder came through the decoder's skip and input gradients."""
    suite.the_join_itself(FORM, WORST, runs(preset, residual, img, n), (preset, residual, img, n))


@pytest.mark.parametrize("preset,residual,img,n", [("ppo", 1, 64, 3), ("segmenter", 0, 96, 2), ("ppo", 1, 32, 129)])
def test_bitwise_against_the_two_single_passes(runs, preset, residual, img, n):
    suite.bitwise_against_the_single_passes(FORM, runs(preset, residual, img, n), (preset, residual, img, n))


@pytest.mark.parametrize("preset,residual,img,n", [("ppo", 1, 96, 2), ("ppo", 1, 32, 129)])
def test_no_stale_reads_and_nothing_outside_the_reported_sizes(runs, preset, residual, img, n):
    """The native calls on guarded buffers of exactly the queried sizes, and the backward again after everything it may only
    write, and the forward's outputs, have been filled with NaNs
    (suite.no_stale_reads_and_nothing_outside_the_reported_sizes)."""
    case = (preset, residual, img, n)
    suite.no_stale_reads_and_nothing_outside_the_reported_sizes(FORM, runs(*case), case)


def test_errors(nets, runs):
    from occlusionenv_amd.encoder import FrozenEncoder
    from tests.segmenter_model import golden_seg_state_dict

    import numpy as np

    sd32, _enc = nets["ppo", 1]
    r = runs("ppo", 1, 64, 3)
    with pytest.raises(ValueError, match="dilation 1 only"):
        TrainableFullNetwork.from_encoder(FrozenEncoder.from_state_dict(sd32, preset="ppo"))  # the preset's dilation 2
    sep = {k: v.float() for k, v in golden_seg_state_dict(np.load(m.GOLDEN), "ppo").items()}
    with pytest.raises(ValueError, match="dense 3x3 convs only"):
        TrainableFullNetwork.from_encoder(FrozenEncoder.from_state_dict(sep, preset="ppo", dilation=1))
    bare = FrozenEncoder.from_state_dict({k: v for k, v in sd32.items() if not k.startswith("segmenter.")}, preset="ppo", dilation=1)
    with pytest.raises(ValueError, match="no segmentation decoder"):
        TrainableFullNetwork.from_encoder(bare)
    suite.errors_tail(FORM, r)
    # "segmenter": Segmenter.forward's pair without the decoder feature
    seg = TrainableFullNetwork.from_encoder(nets["segmenter", 1][1])
    none, prob = seg(r["obs"])
    assert none is None and prob.shape == (3, 1, 64, 64) and prob.requires_grad and not seg.has_grad_head


@pytest.fixture(scope="module")
def trained(nets):
    """Forty AdamW steps at lr 1e-3 on a fixed batch (N=4, S=64), Dice + MSE as in pretrainer.py."""
    return suite.trained_joint(FORM, nets["ppo", 1][1])


def test_learning(trained):
    print("Dice + MSE:", [f"{v:.4f}" for v in trained["losses"][::5]])
    suite.learning(FORM, trained)


def test_round_trip_into_a_frozen_encoder(trained):
    net, enc, obs = trained["net"], trained["enc"], trained["obs"]
    sd = net.state_dict()
    assert len(sd) == 16 * 6 + 5 * 6 + 2 + 2 and "segmenter.0.features.0.up.conv.weight" in sd and "gradPredictor.bias" in sd
    tuned = enc.with_encoder(sd).with_decoder(sd)
    with torch.no_grad():
        pooled, segm, pred = net(obs)
    f2, s2, g2 = tuned.forward_full(obs)
    assert torch.equal(f2, pooled) and torch.equal(s2, segm)
    assert torch.allclose(g2, pred, rtol=1e-5, atol=1e-6)  # addmm against F.linear
    both = enc.with_state(sd)
    assert torch.equal(both.segment(obs), segm) and torch.equal(both(obs), pooled)
    assert not torch.equal(enc.segment(obs), segm) and not torch.equal(enc(obs), pooled)  # the source is left as it is


def test_pretrain_epoch(nets):
    suite.pretrain_epoch(FORM, nets["ppo", 1][1])
