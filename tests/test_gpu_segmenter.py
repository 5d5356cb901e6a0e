"""GPU tests of the native segmentation decoder (occlusionenv_amd/encoder.py: segment, forward_full, occlusion_metrics;
csrc/occ_decoder.hpp): against the f64 host model (tests/segmenter_model.py) and the reference's fixture
(tests/golden/segmenter_golden.npz), bitwise reproducibility (repeat calls, batch position, chunking, graph replay, the
pooled feature against the encoder-only path), the accuracy / IoU counts, real observations and the evaluation loop.

Tolerance: logits within TOL * max(1, max |logit64|) and probabilities within TOL = 1e-4, the bar
tests/test_gpu_encoder.py holds the encoder to.  Thresholded maps must equal the f64 map wherever |logit64| is outside
that band (tests/segmenter_model.py: exempt_band)."""
import os

import numpy as np
import pytest
import torch

from tests.encoder_model import make_obs
from tests.segmenter_model import exempt_band, full_forward, golden_seg_state_dict

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "segmenter_golden.npz")
TOL = 1e-4
WORST = {}  # measured worst error per preset (printed with -s)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def nets(golden):
    from occlusionenv_amd.encoder import FrozenEncoder

    out = {}
    for preset in ("ppo", "segmenter"):
        sd = golden_seg_state_dict(golden, preset)
        enc = FrozenEncoder.from_state_dict(sd, preset=preset)
        assert enc.has_decoder
        out[preset] = (sd, enc)
    return out


def _err(got, want):
    scale = max(1.0, float(want.abs().max()))
    return float((got.double().cpu() - want).abs().max()) / scale


def _check_maps(preset, key, prob, logit, logit64, max_exempt=None):
    """Logits, probabilities and the thresholded map against f64 logits; returns the exempt share."""
    el = _err(logit, logit64)
    ep = float((prob.double().cpu() - torch.sigmoid(logit64)).abs().max())
    band = exempt_band(logit64)
    share = float(band.double().mean())
    WORST[preset] = max(WORST.get(preset, 0.0), el, ep)
    print(f"{preset} {key}: logits {el:.3g}, prob {ep:.3g}, exempt share {share:.3g} (worst so far {WORST[preset]:.3g})")
    assert prob.shape == logit64.shape and prob.dtype == torch.float32
    assert el <= TOL and ep <= TOL, (preset, key, el, ep)
    differ = (prob.cpu() > 0.5) != (logit64 > 0)
    assert not bool((differ & ~band).any()), (preset, key, int((differ & ~band).sum()))
    if max_exempt is not None:
        assert share <= max_exempt, (preset, key, share)
    return share


CASES = [(64, 1), (64, 5), (64, 64), (96, 3), (128, 5), (256, 2), (512, 1)]


@pytest.mark.parametrize("preset", ["ppo", "segmenter"])
@pytest.mark.parametrize("img,n", CASES)
def test_against_f64_host_model(nets, preset, img, n):
    sd, enc = nets[preset]
    obs64 = make_obs(2000 + img + n, n, img)
    want = full_forward(sd, obs64, preset)
    obs = obs64.float().cuda()
    feats, prob, logit = enc.segment(obs, return_logits=True, return_features=True)
    assert feats.shape == (n, 8, img, img) and logit.shape == (n, 1, img, img)
    _check_maps(preset, f"S={img} N={n}", prob, logit, want["logit"])
    ef = _err(feats, want["features"])
    assert ef <= TOL, (preset, img, n, ef)
    if preset == "ppo":
        pooled, segm, grad = enc.forward_full(obs)
        assert pooled.shape == (n, 256) and grad.shape == (n, 2) and torch.equal(segm, prob)
        assert _err(pooled, want["pooled"]) <= TOL and _err(grad, want["grad"]) <= TOL
    else:
        with pytest.raises(ValueError, match="no gradPredictor"):
            enc.predict_grad(obs)


@pytest.mark.parametrize("preset", ["ppo", "segmenter"])
def test_against_reference_fixture(golden, nets, preset):
    _sd, enc = nets[preset]
    for n, img, seed in golden["inputs"]:
        obs = make_obs(int(seed), int(n), int(img)).float().cuda()
        key = f"{preset}_logit_{img}"
        logit64 = torch.from_numpy(golden[key] if key in golden.files else golden[key + "_f32"].astype(np.float64))
        out = enc.segment(obs, return_logits=True, return_features=preset == "segmenter")
        prob, logit = out[-2], out[-1]
        # the generator asserted at most 0.1 % of these pixels inside the exempt band
        _check_maps(preset, f"fixture S={img}", prob, logit, logit64, max_exempt=1e-3)
        p64 = torch.from_numpy(golden[f"{preset}_prob_{img}_f32"].astype(np.float64))
        assert float((prob.double().cpu() - p64).abs().max()) <= TOL
        key = f"{preset}_features_{img}_f32"
        if key in golden.files:
            assert _err(out[0], torch.from_numpy(golden[key].astype(np.float64))) <= TOL


@pytest.mark.parametrize("residual,dilation", [(False, 2), (True, 1), (False, 1)])
def test_explicit_configurations(nets, residual, dilation):
    """Any dilation / residual combination given explicitly: the skip tensor is Layer 2's output plus the residual only
    when there is one, so a skip taken before the residual add shows here."""
    from occlusionenv_amd.encoder import FrozenEncoder

    for preset, (sd, _) in nets.items():
        enc = FrozenEncoder.from_state_dict(sd, preset=preset, dilation=dilation, residual=residual)
        obs64 = make_obs(7, 3, 96)
        want = full_forward(sd, obs64, preset, dilation, residual)
        prob, logit = enc.segment(obs64.float().cuda(), return_logits=True)
        _check_maps(preset, f"residual={residual} dilation={dilation}", prob, logit, want["logit"])
    # the residual changes the map by far more than the tolerance: the case above can tell the two apart
    sd, _ = nets["ppo"]
    a = full_forward(sd, make_obs(7, 3, 96), "ppo", 2, True)["logit"]
    b = full_forward(sd, make_obs(7, 3, 96), "ppo", 2, False)["logit"]
    assert float((a - b).abs().max()) > 100 * TOL


def _batch64():
    g = torch.Generator().manual_seed(3)
    base = make_obs(11, 8, 128).float()
    batch = base[torch.randint(0, 8, (64,), generator=g)] * (0.5 + torch.rand(64, 1, 1, 1, generator=g))
    batch[:, 3] = base[torch.randint(0, 8, (64,), generator=g)][:, 3]
    return batch.cuda()


@pytest.mark.parametrize("preset", ["ppo", "segmenter"])
def test_pooled_feature_is_bitwise_the_encoders(nets, preset):
    """ppo: residual, separable, dilation 2; segmenter: residual, dense, dilation 1; and both without the residual."""
    from occlusionenv_amd.encoder import FrozenEncoder

    sd, enc = nets[preset]
    batch = _batch64()[:9]
    for e in (enc, FrozenEncoder.from_state_dict(sd, preset=preset, residual=False)):
        feats = e._segment(batch, False, False)[0]
        assert torch.equal(feats, e(batch))
        if preset == "ppo":
            assert torch.equal(e.forward_full(batch)[0], e(batch))
    odd = make_obs(5, 2, 100).float().cuda()  # the encoder alone keeps accepting any size
    assert enc(odd).shape == (2, 256)
    with pytest.raises(ValueError, match="multiple of 32"):
        enc.segment(odd)


def test_bitwise_reproducible(nets):
    _sd, enc = nets["ppo"]
    batch = _batch64()
    feats, a, logits = enc.segment(batch, return_logits=True, return_features=True)
    assert torch.equal(enc.segment(batch), a)
    pooled, segm, grad = enc.forward_full(batch)
    assert torch.equal(segm, a) and torch.equal(pooled, enc(batch)) and torch.equal(grad, enc.predict_grad(batch))
    # the optional outputs change no bit of the probabilities (nor of each other)
    f2, p2 = enc.segment(batch, return_features=True)
    p3, l3 = enc.segment(batch, return_logits=True)
    assert torch.equal(p2, a) and torch.equal(p3, a) and torch.equal(f2, feats) and torch.equal(l3, logits)
    # env i alone == env i at any position of a batch of 64
    for i in (0, 17, 63):
        assert torch.equal(enc.segment(batch[i:i + 1])[0], a[i])
        perm = torch.roll(torch.arange(64), 29 + i)
        assert torch.equal(enc.segment(batch[perm]), a[perm])
    # chunking changes no bit
    for chunk in (1, 7, 64):
        enc.max_chunk = chunk
        try:
            assert torch.equal(enc.segment(batch), a), chunk
            assert torch.equal(enc.forward_full(batch)[0], pooled), chunk
        finally:
            enc.max_chunk = 256
    # non-contiguous input
    nc = batch.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not nc.is_contiguous() and torch.equal(enc.segment(nc), a)


def test_graph_capture_matches_eager(nets):
    _sd, enc = nets["ppo"]
    obs = make_obs(21, 16, 128).float().cuda()
    eager = enc.forward_full(obs)  # also creates the workspace of this size
    static = obs.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enc.forward_full(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = enc.forward_full(static)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(o, e) for o, e in zip(out, eager))
    other = make_obs(22, 16, 128).float().cuda()
    static.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(o, e) for o, e in zip(out, enc.forward_full(other)))


def _reference_metrics(pred, target):
    """pretrainer.py:133-141 on a batch, in torch: both maps thresholded, sums over the batch, then the ratios."""
    p, t = pred.reshape(pred.shape[0], -1) > 0.5, target.reshape(target.shape[0], -1) > 0.5
    correct, inter, union = (p == t).sum(1), (p & t).sum(1), (p | t).sum(1)
    acc = correct.sum().double() / float(p.numel())
    iou = inter.sum().double() / union.sum().double()
    return correct, inter, union, acc, iou


def test_metrics_against_torch_sums(nets):
    _sd, enc = nets["ppo"]
    g = torch.Generator().manual_seed(5)
    for n, img in ((6, 64), (3, 96), (2, 512), (70, 32)):
        pred = torch.rand(n, 1, img, img, generator=g).cuda()
        target = (torch.rand(n, img, img, generator=g) * 1.2).cuda()
        target[0] = pred[0, 0]  # an env whose prediction equals its target: IoU 1
        if n > 2:
            target[1] = 0.0  # nothing occluded
            pred[2] = 0.25  # nothing predicted, with an empty target below: union 0
            target[2] = 0.5  # exactly the threshold is not above it
        for tgt in (target, target[:, None]):
            m = enc.occlusion_metrics(pred, tgt)
            correct, inter, union, acc, iou = _reference_metrics(pred, target)
            assert m["correct"].dtype == torch.int64 and m["correct"].is_cuda and m["correct"].shape == (n,)
            assert torch.equal(m["correct"], correct) and torch.equal(m["intersection"], inter) and torch.equal(m["union"], union)
            assert float(m["accuracy"]) == float(acc) and float(m["iou"]) == float(iou)
        assert int(inter[0]) == int(union[0]) > 0
        if n > 2:
            assert int(inter[1]) == 0 and int(union[2]) == 0 and int(correct[2]) == img * img
    # all-empty batch: 0 / 0 is nan, as in the reference
    zeros = torch.zeros(2, 64, 64, device="cuda")
    m = enc.occlusion_metrics(zeros[:, None], zeros)
    assert torch.isnan(m["iou"]) and float(m["accuracy"]) == 1.0 and int(m["union"].sum()) == 0
    # a strided target (the alpha channel of an (N,S,S,4) image) is read in place
    fs = torch.rand(4, 64, 64, 4, generator=g).cuda()
    pred = torch.rand(4, 1, 64, 64, generator=g).cuda()
    m = enc.occlusion_metrics(pred, fs[..., 3])
    correct, inter, union, acc, iou = _reference_metrics(pred, fs[..., 3].contiguous())
    assert torch.equal(m["correct"], correct) and torch.equal(m["intersection"], inter) and torch.equal(m["union"], union)
    assert float(m["iou"]) == float(iou)


def test_cpu_tensor_and_missing_decoder_raise(golden, nets):
    from occlusionenv_amd._native import NativeError
    from occlusionenv_amd.encoder import FrozenEncoder

    enc = nets["ppo"][1]
    with pytest.raises(NativeError):
        enc.segment(torch.zeros(1, 4, 64, 64))
    with pytest.raises(NativeError):
        enc.occlusion_metrics(torch.zeros(1, 1, 64, 64), torch.zeros(1, 64, 64))
    sd = {k: v for k, v in nets["ppo"][0].items() if not k.startswith("segmenter.")}
    bare = FrozenEncoder.from_state_dict(sd, preset="ppo")
    obs = make_obs(1, 1, 64).float().cuda()
    assert not bare.has_decoder and torch.equal(bare(obs), enc(obs))
    with pytest.raises(ValueError, match="no segmentation decoder"):
        bare.segment(obs)
    with pytest.raises(ValueError, match="no segmentation decoder"):
        bare.forward_full(obs)


@pytest.fixture(scope="module")
def ds():
    from occlusionenv_amd.meshes import SyntheticShapeNet

    return SyntheticShapeNet(n_models=8, seed=1234)


def _venv(ds, N, S, seed=77):
    from environment import OcclusionEnv
    from occlusionenv_amd import environment
    from SubProcVecEnv import SimpleVecEnv

    environment.seed_scene_rng(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return SimpleVecEnv([lambda: OcclusionEnv(ds, img_size=S) for _ in range(N)])


@pytest.mark.parametrize("img", [128, 256])
def test_real_observations(nets, ds, img):
    """obs of a SimpleVecEnv step (depth -1 on the background) against the host model."""
    sd, enc = nets["ppo"]
    venv = _venv(ds, 4, img)
    venv.reset()
    obs, _r, _d, _i = venv.step(torch.zeros(4, 2, device="cuda"))
    obs = obs[:, 0] if obs.dim() == 5 else obs
    assert obs.shape == (4, 4, img, img) and float(obs[:, 3].min()) == -1.0
    want = full_forward(sd, obs.double().cpu(), "ppo")
    prob, logit = enc.segment(obs, return_logits=True)
    _check_maps("ppo", f"real obs S={img}", prob, logit, want["logit"])
    venv.engine.check_status()


def test_evaluate_segmentation(nets, ds):
    """Three steps on 16 envs: the percentages equal those recomputed from the host model's maps on the same observations
    and occlusion images (thresholded maps can only differ inside the exempt band, and those pixels are accounted for)."""
    from occlusionenv_amd import harness

    sd, enc = nets["ppo"]
    seen = []
    orig = enc.forward_full

    def spy(obs):
        seen.append(obs.clone())
        return orig(obs)

    targets = []
    orig_metrics = enc.occlusion_metrics

    def spy_metrics(pred, target):
        targets.append(target.clone())
        return orig_metrics(pred, target)

    enc.forward_full, enc.occlusion_metrics = spy, spy_metrics
    try:
        res = harness.evaluate_segmentation(_venv(ds, 16, 128), enc, 3)
    finally:
        del enc.forward_full, enc.occlusion_metrics
    assert len(seen) == 3 and len(targets) == 3 and res["pixels"] == 3 * 16 * 128 * 128
    assert np.isfinite(res["accuracy"]) and 0.0 <= res["accuracy"] <= 100.0
    correct = inter = union = exempt = 0
    for obs, tgt in zip(seen, targets):
        assert tgt.shape == (16, 128, 128)
        logit64 = full_forward(sd, obs.double().cpu(), "ppo")["logit"][:, 0]
        p, t = logit64 > 0, tgt.cpu() > 0.5
        exempt += int(exempt_band(logit64).sum())
        correct += int((p == t).sum())
        inter += int((p & t).sum())
        union += int((p | t).sum())
    print(f"evaluate_segmentation: {res}, exempt pixels {exempt}")
    # every exempt pixel may move each count by one
    assert abs(res["correct"] - correct) <= exempt and abs(res["intersection"] - inter) <= exempt
    assert abs(res["union"] - union) <= exempt
    if exempt == 0:
        assert res["accuracy"] == 100.0 * correct / res["pixels"]
        assert (res["iou"] == 100.0 * inter / union) if union else np.isnan(res["iou"])
    assert union > 0 and np.isfinite(res["iou"])


