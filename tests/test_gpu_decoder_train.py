"""GPU tests of the native decoder backward (csrc/occ_decoder_bwd.hpp, occlusionenv_amd/seghead.py, harness.
finetune_segmentation) against tests/train_model.py (a ``Net`` with ``frozen_encoder``) in f64 on the CPU: the encoder run once
without autograd, the decoder and the classifier with requires_grad tensors, torch autograd supplying the gradients.  The
bodies this module shares with the other training modules are in tests/train_gpu_suite.py; FORM below is what they are given.

Weights: the fixture's seeded state dict rounded to f32 (what a checkpoint on disk holds, and what the head's f32
parameters can represent), used as exactly those values in f64 by the host model.  Inputs: encoder_model.make_obs.

Shapes (the smallest that reach every code path): S=32 N=1 (deepest level 1x1: every neighbour is the zero edge; one tile per
level), S=64 N=3 (several envs in the K split of the weight gradient), S=96 N=2 (H = 3, 6, 12, 24, 48: partial 4-, 8- and
16-tiles); preset "ppo" on all three, "segmenter" on S=64.  In all of these a block of the weight gradient
(occ_dec_bwd_dw_kernel) owns one pixel tile.  The split cases give it a slice of several (tests/decoder_split_model.py, whose
reach is asserted without a GPU in tests/test_decoder_train_host.py): "ppo" S=96 N=65 has 2, 2, 2, 2, 5 tiles per slice on
levels 0 to 4, a short last slice on levels 0, 2 and 3 and slices that cross an env boundary on levels 2 to 4 (9 and 36 tiles
per env); "segmenter" S=64 N=130 has 3, 1, 2, 2, 5 with a short last slice on level 0 (the dense preset's f64 encode is
cheap, so the large N is there).  At "ppo" S=96 N=65 the backward also runs with an upstream gradient in one env alone,
where a tile given to the wrong env or dropped from the last slice is the whole signal; at "segmenter" S=64 N=130 it runs
through the C entry points on guarded buffers of exactly the queried sizes, and again after everything it may only write was
filled with NaNs; at "ppo" S=64 N=3 with the classifier scaled until the stored f32 p is exactly 0 or 1.

Bars.  Kept relu outputs: within 1e-4 max(1, max |r64|) of the f64 relu(u).  Gates r > 0: may differ from the f64 gate only
where |u64| <= 1e-4 max(1, max |u64|), on at most 1e-3 of the elements; the band itself holds at most 1e-3 of the elements
for these seeds (asserted).  Gradients: per tensor max |got - want| <= 1e-4 max |want| (no floor), the oracle evaluated with
the GPU's own gate (relu(u) replaced by u * gate), so that a flipped borderline pixel is judged by the gate test and not
smeared into every weight sum.

Measured on an MI355X against the f64 model (worst relative error per tensor kind; the bar is 1e-4):
                     conv.weight  conv.bias  bn.weight  bn.bias  classifier weight  bias
  one tile per block   8.8e-7      5.6e-7     1.5e-6    5.5e-7       5.1e-7        1.8e-7
  split cases          7.2e-7      7.5e-7     7.1e-7    5.3e-7       2.1e-7        1.8e-7
  one env alone        1.3e-6      3.2e-7     7.9e-7    5.8e-7       1.1e-7        2.4e-8
  saturated p          1.5e-6      3.3e-7     3.3e-7    2.5e-7       6.6e-8        8.2e-8
Kept relu outputs at the split cases: 1.9e-6; one gate differed from the f64 gate ("ppo" S=96 N=65, level 1), inside the
band.  Largest band share 3.7e-4 and 4.1e-4.  With `env` taken from the slice's first tile, or with the tile loop ended after
one tile, every gradient test of the split cases and both one-env tests fail and every one-tile case still passes."""
import ctypes as C

import numpy as np
import pytest
import torch

from occlusionenv_amd.seghead import SegmentationHead
from tests import criterion_model, decoder_split_model
from tests import train_gpu_suite as suite
from tests import train_model as m
from tests.segmenter_model import PRESETS, golden_seg_state_dict
from tests.train_utils import dice64, grads

pytestmark = pytest.mark.gpu

TOL = 1e-4
SPLIT_CASES = [("ppo", 96, 65), ("segmenter", 64, 130)]  # several tiles per block of the weight gradient, see the docstring
assert SPLIT_CASES == decoder_split_model.SPLIT_CASES  # what they reach is asserted on the host (test_decoder_train_host.py)
CASES = [("ppo", 32, 1), ("ppo", 64, 3), ("ppo", 96, 2), ("segmenter", 64, 3)] + SPLIT_CASES
IDS = [f"{p}-S{s}-N{n}" for p, s, n in CASES]
WORST = {}  # measured worst relative error per tensor kind (printed with -s)


FORM = suite.Form(
    net=SegmentationHead, model=lambda case: m.frozen_net(case[0]),
    symbols=("occ_segment_train_workspace_query", "occ_segment_train_forward", "occ_segment_backward"),
    label=lambda case: "{} S={} N={}".format(*case), n_params=22, seed=4000, steps=5, tol=TOL,
    one_env_seed=2, host_obs_f64=True, band_cap=1e-3, gate_cap=1e-3)


@pytest.fixture(scope="module")
def nets():
    from occlusionenv_amd.encoder import FrozenEncoder

    g = np.load(m.GOLDEN)
    out = {}
    for preset in ("ppo", "segmenter"):
        sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in golden_seg_state_dict(g, preset).items()}
        out[preset] = (sd32, FrozenEncoder.from_state_dict(sd32, preset=preset))
    return out


@pytest.fixture(scope="module")
def runs(nets):
    """Per case, computed once and left unchanged: one native forward + backward with a seeded randn upstream gradient, the
    kept relu outputs, and the host model."""
    return suite.make_runs(FORM, nets)


def _target(case):
    """The case's random occlusion map: drawn behind the fixture's upstream gradient, from its generator."""
    img, n = case[-2:]
    gen = torch.Generator().manual_seed(suite.case_seed(FORM, case) + 1)
    torch.randn(n, 1, img, img, generator=gen)
    return (torch.rand(n, 1, img, img, generator=gen) > 0.5).float()


@pytest.mark.parametrize("preset,img,n", CASES, ids=IDS)
def test_forward_identity(runs, preset, img, n):
    suite.forward_identity(FORM, runs(preset, img, n), (preset, img, n))


@pytest.mark.parametrize("preset,img,n", CASES, ids=IDS)
def test_kept_relu_and_gate(runs, preset, img, n):
    suite.kept_relu_and_gates(FORM, runs(preset, img, n), (preset, img, n))


@pytest.mark.parametrize("preset,img,n", CASES, ids=IDS)
def test_gradients_against_f64_autograd(runs, preset, img, n):
    suite.gradients_against_f64_autograd(FORM, WORST, runs(preset, img, n), (preset, img, n))


@pytest.mark.parametrize("loss", ["dice", "bce"])
@pytest.mark.parametrize("preset,img,n", CASES, ids=IDS)
def test_gradients_through_the_losses(runs, preset, img, n, loss):
    case = (preset, img, n)
    suite.gradients_through_the_real_losses(FORM, WORST, runs(*case), case, loss, occl=_target(case))


def test_reproducible_overwrite_and_accumulation(runs):
    from occlusionenv_amd import _native as nat
    from occlusionenv_amd.encoder import decoder_packed_floats

    r = runs("ppo", 64, 3)
    suite.reproducible_and_accumulating(r)
    # the native call overwrites grad_packed: garbage in the buffer changes no bit
    n, img = 3, 64
    head, enc, up = r["net"], r["enc"], r["ups"][0].cuda()
    ws, scratch = head._train_buffers(n, img)
    outs = []
    for fill in (0.0, 123.0):
        gp = torch.full((decoder_packed_floats(),), fill, device="cuda")
        nat.check(nat.load().occ_segment_backward(C.byref(enc._cfg(img)), nat.ptr(enc.dec_packed), n, nat.ptr(ws), ws.numel(),
                                                  nat.ptr(up), nat.ptr(scratch), scratch.numel(), nat.ptr(gp),
                                                  nat.stream_ptr(up.device)), "occ_segment_backward")
        outs.append(gp)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


@pytest.mark.parametrize("env", [64, 1])
def test_gradients_of_one_env(runs, env):
    """The upstream gradient is randn in one env and zero in the others, so that env's tiles are the whole signal: env 64
    alone fills the short last slice of level 0; env 1 is where the first slices that cross an env boundary on levels 2 to
    4 end (asserted on the host model, test_decoder_train_host.py)."""
    suite.gradients_of_one_env(FORM, WORST, runs(*SPLIT_CASES[0]), SPLIT_CASES[0], env)


def test_no_stale_reads_and_nothing_outside_the_reported_sizes(runs):
    """The native calls on guarded buffers of exactly the queried sizes, and the backward again after everything it may only
    write (scratch, the two gradient buffers at the end of the workspace, grad_packed) and the forward's outputs have been
    filled with NaNs (suite.no_stale_reads_and_nothing_outside_the_reported_sizes)."""
    suite.no_stale_reads_and_nothing_outside_the_reported_sizes(FORM, runs(*SPLIT_CASES[1]), SPLIT_CASES[1])


@pytest.mark.parametrize("loss", ["dice", "bce"])
@pytest.mark.parametrize("factor", [64, 512])
def test_saturated_probabilities(runs, factor, loss):
    """Classifier weight and bias times ``factor``: the stored f32 p is exactly 1 (and, at 512, exactly 0) on many pixels.
    The contract is dz = g p (1 - p) from the stored p, so dz = 0 there although BCE's g is of order 1e12 x coef: the oracle
    takes the GPU's p, g from criterion_model at that p, dz in f64, and back-propagates sum(logit dz) through the host model.

    1 / (1 + expf(-z)) is exactly 1 for z > 17.4 and exactly 0 only once expf overflows, z < -88.8.  This case's logits lie
    in [-0.262, 1.102], so 64 saturates the upper end only ([-16.8, 70.5]); 512 ([-134, 564]) saturates both."""
    from occlusionenv_amd import segmentation

    case = preset, img, n = "ppo", 64, 3
    r = runs(*case)
    sd, cls = dict(r["sd"]), PRESETS[preset]["classifier"]
    head = SegmentationHead.from_encoder(r["enc"])
    with torch.no_grad():
        for t in ("weight", "bias"):
            head.get_parameter(cls + t).mul_(float(factor))
            sd[cls + t] = sd[cls + t] * float(factor)  # a power of two: the same values in f32 and in f64
    target = _target(case)
    prob = head(r["obs"])
    p32 = prob.detach().cpu()
    one, zero = p32 == 1.0, p32 == 0.0
    print(f"factor {factor}: {int(one.sum())} pixels with p == 1, {int(zero.sum())} with p == 0, of {p32.numel()}")
    assert bool((target[one] == 1).any()) and bool((target[one] == 0).any())
    if factor == 512:
        assert bool((target[zero] == 1).any()) and bool((target[zero] == 0).any())
    native = segmentation.binary_dice_loss if loss == "dice" else segmentation.binary_cross_entropy
    native(prob, target.cuda()).backward()
    got = grads(head)
    assert len(got) == 22 and all(bool(torch.isfinite(v).all()) for v in got.values())
    g = (criterion_model.dice_grad if loss == "dice" else criterion_model.bce_grad)(p32, target)
    dz = g * p32.double() * (1.0 - p32.double())
    assert bool((dz[one] == 0).all()) and bool((dz[zero] == 0).all())
    host = m.HostModel(sd, FORM.model(case), r["obs"].double().cpu())
    _pooled, logit = host.logit(suite.gates_of(head))
    want = host.grads((logit * dz).sum())
    suite.check_grads(FORM, WORST, f"saturated x{factor} {loss} {preset} S={img} N={n}", case, got, want)


@pytest.fixture(scope="module")
def trained(runs):
    """Five AdamW steps at lr 1e-3 on a fixed batch (S=64, N=3): the f64 host model first, then the native head."""
    from occlusionenv_amd import segmentation

    case = ("ppo", 64, 3)
    r, occl = runs(*case), _target(case)
    host = m.HostModel(r["sd"], FORM.model(case), r["obs"].double().cpu())
    opt = torch.optim.AdamW(list(host.params.values()), lr=1e-3, weight_decay=1e-5)
    host_losses = []
    for _ in range(FORM.steps + 1):  # five steps, and the loss after the fifth
        opt.zero_grad()
        loss = dice64(host.forward()[1], occl)
        host_losses.append(float(loss.detach()))
        if len(host_losses) <= FORM.steps:
            loss.backward()
            opt.step()
    head, target = SegmentationHead.from_encoder(r["enc"]), occl.cuda()
    before, losses = suite.train(FORM, head, lambda net: segmentation.binary_dice_loss(net(r["obs"]), target), weight_decay=1e-5)
    return dict(net=head, before=before, host_losses=host_losses, losses=losses, obs=r["obs"], enc=r["enc"], prob0=r["outs"][-1])


def test_learning(trained):
    print("host Dice:", trained["host_losses"], "native Dice:", trained["losses"])
    assert trained["host_losses"][-1] < trained["host_losses"][0]
    suite.learning(FORM, trained)


def test_round_trip_into_a_frozen_encoder(trained):
    from occlusionenv_amd.encoder import DECODER_KEYS

    head, enc, obs = trained["net"], trained["enc"], trained["obs"]
    sd = head.state_dict()
    dp, dc = DECODER_KEYS["ppo"]
    assert dp + "0.up.conv.weight" in sd and dp + "4.up.bn.running_var" in sd and dc + "bias" in sd
    assert tuple(sd[dp + "0.up.conv.weight"].shape) == (256, 128, 3, 3)
    assert all(k.startswith("ckpt.") for k in head.state_dict(prefix="ckpt."))
    tuned = enc.with_decoder(sd)
    with torch.no_grad():
        now = head(obs)
    assert torch.equal(tuned.segment(obs), now)
    assert not torch.equal(now, trained["prob0"])
    assert torch.equal(enc.segment(obs), trained["prob0"])  # the untouched encoder keeps its map
    assert torch.equal(tuned(obs), enc(obs))


def test_errors(nets, runs):
    from occlusionenv_amd.encoder import FrozenEncoder

    sd, _enc = nets["ppo"]
    bare = FrozenEncoder.from_state_dict({k: v for k, v in sd.items() if not k.startswith("segmenter.")}, preset="ppo")
    with pytest.raises(ValueError, match="no segmentation decoder"):
        SegmentationHead.from_encoder(bare)
    suite.errors_tail(FORM, runs("ppo", 64, 3))


def test_finetune_segmentation_harness(nets):
    from environment import OcclusionEnv
    from occlusionenv_amd import environment, harness
    from occlusionenv_amd.meshes import SyntheticShapeNet
    from SubProcVecEnv import SimpleVecEnv

    ds = SyntheticShapeNet(n_models=8, seed=1234)
    environment.seed_scene_rng(77)
    np.random.seed(77)
    torch.manual_seed(77)
    venv = SimpleVecEnv([lambda: OcclusionEnv(ds, img_size=128) for _ in range(16)])
    head = SegmentationHead.from_encoder(nets["ppo"][1])
    before = {k: v.detach().clone() for k, v in head.named_parameters()}
    res = harness.finetune_segmentation(venv, head, 3)
    assert res["head"] is head and res["steps"] == 3
    for key in ("losses", "accuracy", "iou"):
        assert len(res[key]) == 3
    assert all(np.isfinite(v) for v in res["losses"]) and all(0.0 <= v <= 100.0 for v in res["accuracy"])
    assert all(not torch.equal(v, before[k]) for k, v in head.named_parameters())
    # from an encoder: a head is made, with BCE
    res = harness.finetune_segmentation(venv, nets["ppo"][1], 1, use_dice=False)
    assert isinstance(res["head"], SegmentationHead) and np.isfinite(res["losses"][0])
