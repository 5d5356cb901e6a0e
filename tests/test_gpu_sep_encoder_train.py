"""GPU tests of the native separable-encoder backward (csrc/occ_sepenc_bwd.hpp, occlusionenv_amd/septrain.py,
harness.train_predictor) against tests/sep_encoder_train_model.py in f64 on the CPU, torch autograd supplying the gradients.

Weights, rounded to f32 (what a checkpoint on disk holds) and used as exactly those values in f64 by the host model:
"golden" = the separable FullNetwork fixture tests/golden/encoder_golden.npz ("ppo" keys) whose inference is pinned to the
reference, run at dilation 2 with the residual and once at dilation 1 with the residual; "predictor" =
sep_encoder_train_model.sep_state_dict("predictor", 32, gain 1.25) at dilation 1 without the residual, tanh head.  Inputs:
encoder_model.make_obs; the upstream grad_feats is randn.

Shapes: S=32 N=2 (the deepest planes are 2x2 and 1x1: a dilation-2 halo is all padding), S=40 N=3 (sides 40 / 20 / 10 / 5 / 3 /
2: odd sides, 8- and 16-pixel tiles, ragged last tiles), S=96 N=2 (several 16-pixel tiles per side: a dilation-2 halo crosses
tile boundaries).  In all of these a block of the pointwise weight gradient owns one pixel tile.  The split case S=33 N=115
(golden weights, dilation 2) gives it 2 tiles per slice on the initial layer and on both layers of levels 0 and 1, 9 tiles per
env, with a last slice of one tile and slices that cross env boundaries (asserted without a GPU in
tests/test_sep_encoder_train_host.py); there the backward also runs with an upstream gradient in one env alone (the last env,
which holds the short last slice, and env 1, where the first slice that crosses an env boundary ends), and through the C entry
points on guarded buffers of exactly the queried sizes, again after everything it may only write was filled with NaNs.

Bars (the dense tests', tests/test_gpu_encoder_train.py).  Kept relu outputs: within 1e-4 max(1, max |r64|) of the f64
relu(u).  Gates r > 0: may differ from the f64 gate only where |u64| <= 1e-4 max(1, max |u64|); that band holds at most 1 % of
any layer's pixels (asserted).  Gradients: per tensor max |got - want| <= 1e-4 max |want| (no floor; no tensor's gradient is
all zero), the oracle evaluated with the GPU's own gates.

Measured on an MI355X against the f64 model (worst relative error per tensor kind; the bar is 1e-4):
                      conv.0.w  conv.1.w  conv.2.w  conv.2.bias  bn.weight  bn.bias  down conv.w  down conv.bias  head w  head bias
  one tile per block   2.4e-6    2.7e-6    2.2e-6     1.7e-6      4.8e-6    1.5e-6    2.5e-6       9.4e-7
  through head + MSE   6.2e-6    4.7e-6    9.9e-6     1.0e-5      5.8e-6    1.3e-5    2.6e-6       2.6e-6      7.2e-7   7.3e-7
  split case           8.2e-7    1.9e-6    1.2e-6     1.7e-6      1.1e-6    1.1e-6    6.5e-7       6.9e-7
  one env alone        2.8e-6    1.6e-6    1.3e-6     8.6e-7      7.4e-7    7.1e-7    5.3e-7       4.8e-7
Kept relu outputs: 2.0e-6; no gate differed from the f64 gate in any case; worst band share 0.40 %.  Checked by hand with
in-bounds mutations of the kernels: the dPW tile loop ended after one tile fails the split case's gradient test and both
one-env tests; the env taken from the slice's first tile fails the split case's gradient test and the one-env test of env 1
(no slice crosses into the last env, so that test passes); the dX stencil offset taken at dilation 1 fails every d = 2
gradient test; each passes every other case.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import sep_encoder_train_model as m
from tests.encoder_model import golden_state_dict, make_obs
from tests.train_utils import GUARD
from tests.train_utils import grads as _grads
from tests.train_utils import guarded as _guarded

pytestmark = pytest.mark.gpu

TOL = 1e-4
BAND_CAP = 0.01
SPLIT = ("golden", 2) + m.SPLIT_CASE
SMALL = [(w, d, s, n) for s, n in ((32, 2), (40, 3), (96, 2)) for w, d in (("golden", 2), ("predictor", 1))] + [("golden", 1, 40, 3)]
CASES = SMALL + [SPLIT]
IDS = [f"{w}-d{d}-S{s}-N{n}" for w, d, s, n in CASES]
WORST = {}  # measured worst relative error per tensor kind (printed with -s)


def _seed(img, n):
    return 9000 + img + n


@pytest.fixture(scope="module")
def nets():
    """(weights, dilation) -> (sd32, sd64, preset, FrozenEncoder)."""
    from occlusionenv_amd.encoder import FrozenEncoder

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_golden.npz"))
    golden = {k: v.float() for k, v in golden_state_dict(g, "ppo").items()}
    pred = {k: v.float() for k, v in m.sep_state_dict("predictor", 32, gain=1.25).items()}
    out = {}
    for wname, d, sd32, preset in (("golden", 2, golden, "ppo"), ("golden", 1, golden, "ppo"), ("predictor", 1, pred, "predictor")):
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd32.items()}
        enc = FrozenEncoder.from_state_dict(sd32, preset=preset, dilation=d)
        assert enc.separable and enc.dilation == d and enc.residual == (preset == "ppo")
        out[(wname, d)] = (sd32, sd64, preset, enc)
    return out


@pytest.fixture(scope="module")
def runs(nets):
    """Per case, computed once and left unchanged: one native forward + backward with a seeded randn upstream gradient, the
    kept relu outputs, and the host model."""
    from occlusionenv_amd.septrain import TrainableSeparableEncoder

    cache = {}

    def get(wname, d, img, n):
        key = (wname, d, img, n)
        if key not in cache:
            _sd32, sd64, preset, enc = nets[(wname, d)]
            obs64 = make_obs(_seed(img, n), n, img)
            obs = obs64.float().cuda()
            net = TrainableSeparableEncoder.from_encoder(enc)
            feats = net(obs)
            up = torch.randn(n, 256, generator=torch.Generator().manual_seed(_seed(img, n) + 1))
            net.zero_grad()
            feats.backward(up.cuda())
            kept = [net._kept_relu(i).cpu().clone() for i in range(16)]
            cache[key] = dict(enc=enc, net=net, obs=obs, feats=feats.detach(), up=up, kept=kept, preset=preset,
                              grads={k: v.cpu() for k, v in _grads(net).items()},
                              host=m.HostModel(sd64, preset, obs.double().cpu(), dilation=d))
        return cache[key]

    return get


def _kind(k):
    for marker in (".conv.", ".bn."):
        if marker in k:
            return k[k.index(marker) + 1:]
    return "head." + k.rsplit(".", 1)[-1]


def _check_grads(what, got, want):
    for k, w in want.items():
        scale = float(w.abs().max())
        assert scale > 0.0, (what, k, "the oracle's gradient is all zero")
        err = float((got[k].double().cpu() - w).abs().max()) / scale
        WORST[_kind(k)] = max(WORST.get(_kind(k), 0.0), err)
        print(f"{what} {k}: max|want| {scale:.3g}, relative error {err:.3g}")
    for k, w in want.items():
        assert got[k].shape == w.shape and got[k].dtype == torch.float32
        assert float((got[k].double().cpu() - w).abs().max()) <= TOL * float(w.abs().max()), (what, k)
    print("worst so far:", {k: f"{v:.3g}" for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("wname,d,img,n", CASES, ids=IDS)
def test_forward_identity(runs, wname, d, img, n):
    r = runs(wname, d, img, n)
    assert r["feats"].shape == (n, 256)
    assert torch.equal(r["feats"], r["enc"](r["obs"]))


@pytest.mark.parametrize("wname,d,img,n", CASES, ids=IDS)
def test_kept_relu_and_gate(runs, wname, d, img, n):
    r = runs(wname, d, img, n)
    us = []
    with torch.no_grad():
        r["host"].feats(None, us)
    total, worst_band = 0, 0.0
    for i, (u64, got) in enumerate(zip(us, r["kept"])):
        assert got.shape == u64.shape
        r64 = torch.relu(u64)
        err = float((got.double() - r64).abs().max()) / max(1.0, float(r64.abs().max()))
        band = u64.abs() <= TOL * max(1.0, float(u64.abs().max()))
        share = float(band.double().mean())
        differ = (got > 0) != (u64 > 0)
        total += int(differ.sum())
        worst_band = max(worst_band, share)
        print(f"{wname} d={d} S={img} N={n} layer {i}: relu error {err:.3g}, band share {share:.3g}, gates differing {int(differ.sum())}")
        assert err <= TOL, (i, err)
        assert share <= BAND_CAP, (i, share)
        assert not bool((differ & ~band).any()), (i, int((differ & ~band).sum()))
    print(f"{wname} d={d} S={img} N={n}: {total} gates differ from the f64 model's, worst band share {worst_band:.3g}")


@pytest.mark.parametrize("wname,d,img,n", CASES, ids=IDS)
def test_gradients_against_f64_autograd(runs, wname, d, img, n):
    r = runs(wname, d, img, n)
    host = r["host"]
    gates = [(k > 0).double() for k in r["kept"]]
    want = host.grads((host.feats(gates) * r["up"].double()).sum())
    assert len(want) == 11 * 6 + 5 * 4 and set(want) <= set(r["grads"])
    _check_grads(f"{wname} d={d} S={img} N={n}", r["grads"], want)


@pytest.mark.parametrize("wname,d,img,n", SMALL, ids=IDS[:len(SMALL)])
def test_gradients_through_the_head_and_mse(runs, wname, d, img, n):
    r = runs(wname, d, img, n)
    net, host = r["net"], r["host"]
    target = torch.randn(n, 2, generator=torch.Generator().manual_seed(_seed(img, n) + 2)).clamp(-1, 1)
    net.zero_grad()
    loss = F.mse_loss(net.predict_grad(r["obs"]), target.cuda())
    loss.backward()
    got = _grads(net)
    gates = [(net._kept_relu(i).cpu() > 0).double() for i in range(16)]
    loss64 = F.mse_loss(host.predict(gates), target.double())
    want = host.grads(loss64, head=True)
    assert len(want) == 11 * 6 + 5 * 4 + 2
    assert abs(float(loss.detach()) - float(loss64.detach())) <= TOL * max(1.0, abs(float(loss64.detach())))
    _check_grads(f"mse {wname} d={d} S={img} N={n}", got, want)


@pytest.mark.parametrize("env", [SPLIT[3] - 1, 1])
def test_gradients_of_one_env(runs, env):
    """The upstream gradient is randn in one env and zero in the others, so that env's tiles are the whole signal."""
    wname, d, img, n = SPLIT
    r = runs(*SPLIT)
    net, host = r["net"], r["host"]
    up = torch.zeros(n, 256)
    up[env] = torch.randn(256, generator=torch.Generator().manual_seed(_seed(img, n) + 3 + env))
    net.zero_grad()
    feats = net(r["obs"])
    assert torch.equal(feats.detach(), r["feats"])
    feats.backward(up.cuda())
    got = _grads(net)
    gates = [(net._kept_relu(i).cpu() > 0).double() for i in range(16)]
    want = host.grads((host.feats(gates) * up.double()).sum())
    _check_grads(f"one-hot env {env} {wname} d={d} S={img} N={n}", got, want)


def test_reproducible_and_accumulating(runs):
    r = runs("golden", 2, 40, 3)
    net, obs, up = r["net"], r["obs"], r["up"].cuda()
    net.zero_grad()
    net(obs).backward(up)
    once = _grads(net)
    assert all(torch.equal(once[k].cpu(), r["grads"][k]) for k in once)  # the same bits as the fixture's call
    net(obs).backward(up)  # without zero_grad the second pass accumulates as torch does: g + g, exact
    assert all(torch.equal(v, once[k] + once[k]) for k, v in _grads(net).items())
    net.zero_grad()


@pytest.mark.parametrize("wname,d,img,n", [SPLIT, ("predictor", 1, 40, 3)], ids=[IDS[-1], IDS[3]])
def test_no_stale_reads_and_nothing_outside_the_reported_sizes(runs, wname, d, img, n):
    """The native calls on buffers of exactly the queried sizes, each the middle of a larger allocation that is inspected
    afterwards; then the backward again after everything it may only write (scratch, the three gradient buffers at the end
    of the workspace, grad_packed) has been filled with NaNs: the same bits, so nothing read was left over from before."""
    from occlusionenv_amd import _native as nat
    from occlusionenv_amd.encoder import packed_floats
    from occlusionenv_amd.septrain import unpack_sep_encoder_buffer

    r = runs(wname, d, img, n)
    enc, net, obs, up = r["enc"], r["net"], r["obs"], r["up"].cuda()
    lib, cfg, st = nat.load(), enc._cfg(img), nat.stream_ptr(obs.device)
    wsb, scb = C.c_size_t(), C.c_size_t()
    nat.check(lib.occ_sep_encoder_train_workspace_query(C.byref(cfg), n, C.byref(wsb), C.byref(scb)),
              "occ_sep_encoder_train_workspace_query")
    sizes = dict(ws=int(wsb.value), scratch=int(scb.value), grad_packed=4 * packed_floats(True), feats=4 * n * 256)
    assert sizes["scratch"] == m.scratch_bytes(img, n)
    bufs = {k: _guarded(b) for k, b in sizes.items()}
    mid = {k: whole[lo:lo + sizes[k]] for k, (whole, lo) in bufs.items()}
    assert all(v.data_ptr() % 256 == 0 for v in mid.values())

    def backward():
        nat.check(lib.occ_sep_encoder_backward(C.byref(cfg), nat.ptr(enc.packed), n, nat.ptr(mid["ws"]), sizes["ws"], nat.ptr(up),
                                               nat.ptr(mid["scratch"]), sizes["scratch"], nat.ptr(mid["grad_packed"]), st),
                  "occ_sep_encoder_backward")
        return mid["grad_packed"].view(torch.float32).clone()

    nat.check(lib.occ_sep_encoder_train_forward(C.byref(cfg), nat.ptr(enc.packed), nat.ptr(obs), n, nat.ptr(mid["ws"]), sizes["ws"],
                                                nat.ptr(mid["feats"]), st), "occ_sep_encoder_train_forward")
    feats = mid["feats"].clone()
    assert torch.equal(feats.view(torch.float32).view(n, 256), r["feats"])
    a = backward()
    again = backward()
    nan = 0x7FC00000
    mid["scratch"].view(torch.int32).fill_(nan)
    tail = 3 * ((4 * n * 8 * img * img + 255) & ~255)  # g0 | g1 | g2, the end of the layout in include/occlusionenv_amd.h
    mid["ws"][sizes["ws"] - tail:].view(torch.int32).fill_(nan)
    mid["grad_packed"].view(torch.int32).fill_(nan)
    b = backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a.view(torch.int32), again.view(torch.int32)) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(mid["feats"], feats)  # the backward does not write it
    # the packed gradient is the module's: the conv weights and biases as they are, the BN affine through the fold
    layers = unpack_sep_encoder_buffer(a.cpu())
    part = net.parts[0]
    for layer, stem, leaves in zip(layers, part.stems, part.layer_leaves()):
        for t, leaf in zip(layer[:-2], leaves[:-2]):
            assert torch.equal(t, r["grads"][stem + leaf]), stem + leaf
    for k, (whole, lo) in bufs.items():
        assert lo >= GUARD and whole.numel() - (lo + sizes[k]) >= GUARD
        assert bool((whole[:lo] == 0xA5).all()), f"bytes in front of {k} were written"
        assert bool((whole[lo + sizes[k]:] == 0xA5).all()), f"bytes behind {k} were written"


@pytest.fixture(scope="module")
def trained(runs):
    """Twenty AdamW steps at lr 1e-3 on a fixed batch ("predictor", S=40, N=3) towards fixed unit targets."""
    from occlusionenv_amd.septrain import TrainableSeparableEncoder

    r = runs("predictor", 1, 40, 3)
    net = TrainableSeparableEncoder.from_encoder(r["enc"])
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    target = F.normalize(torch.randn(3, 2, generator=torch.Generator().manual_seed(5)), dim=1).cuda()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    losses = []
    for _ in range(21):  # twenty steps, and the loss after the twentieth
        opt.zero_grad()
        loss = F.mse_loss(net.predict_grad(r["obs"]), target)
        losses.append(float(loss.detach()))
        if len(losses) <= 20:
            loss.backward()
            opt.step()
    return dict(net=net, before=before, losses=losses, obs=r["obs"], enc=r["enc"], feats0=r["feats"])


def test_learning(trained):
    print("native MSE:", trained["losses"][0], "->", trained["losses"][-1])
    assert all(np.isfinite(v) for v in trained["losses"])
    assert trained["losses"][-1] < trained["losses"][0]
    assert all(not torch.equal(v, trained["before"][k]) for k, v in trained["net"].named_parameters())


def test_round_trip_into_a_frozen_encoder(trained):
    net, enc, obs = trained["net"], trained["enc"], trained["obs"]
    sd = net.state_dict()
    assert "features.initial.conv.0.weight" in sd and "features.features.4.down.bn.running_var" in sd and "output.bias" in sd
    assert tuple(sd["features.features.4.net.Layer 2.conv.0.weight"].shape) == (128, 1, 3, 1)
    assert tuple(sd["features.features.4.net.Layer 2.conv.1.weight"].shape) == (128, 1, 1, 3)
    assert tuple(sd["features.features.4.net.Layer 2.conv.2.weight"].shape) == (128, 128, 1, 1)
    assert tuple(sd["features.features.4.down.conv.weight"].shape) == (256, 128, 3, 3)
    tuned = enc.with_encoder(sd)
    with torch.no_grad():
        now = net(obs)
        grad_now = net.predict_grad(obs)
    assert torch.equal(tuned(obs), now)
    assert not torch.equal(now, trained["feats0"])
    assert torch.equal(enc(obs), trained["feats0"])  # the untouched encoder keeps its feature
    assert torch.allclose(tuned.predict_grad(obs), grad_now, rtol=1e-5, atol=1e-6)  # addmm against F.linear


def test_errors(runs):
    from occlusionenv_amd._native import NativeError
    from occlusionenv_amd.encoder import FrozenEncoder
    from occlusionenv_amd.septrain import TrainableSeparableEncoder
    from tests.encoder_train_model import dense_state_dict

    dense = FrozenEncoder.from_state_dict({k: v.float() for k, v in dense_state_dict("predictor", 32).items()}, preset="predictor")
    assert not dense.separable
    with pytest.raises(ValueError, match="dense"):
        TrainableSeparableEncoder.from_encoder(dense)
    with pytest.raises(ValueError, match="FrozenEncoder"):
        TrainableSeparableEncoder.from_encoder(object())
    r = runs("predictor", 1, 40, 3)
    net, enc = r["net"], r["enc"]
    enc.max_chunk = 2
    try:
        with pytest.raises(ValueError, match="max_chunk"):
            net(r["obs"])
    finally:
        enc.max_chunk = 256
    with pytest.raises(NativeError):
        net(torch.zeros(1, 4, 64, 64))
    first = net(r["obs"])
    second = net(r["obs"][:1])
    with pytest.raises(RuntimeError, match="superseded"):
        first.sum().backward()
    net.zero_grad()
    second.sum().backward()  # the latest forward still has its activations
    assert all(p.grad is not None for k, p in net.named_parameters() if not k.startswith("output."))
    net.zero_grad()


def test_train_predictor_harness(nets):
    from environment import OcclusionEnv
    from occlusionenv_amd import environment, harness
    from occlusionenv_amd.meshes import SyntheticShapeNet
    from occlusionenv_amd.septrain import TrainableSeparableEncoder
    from SubProcVecEnv import SimpleVecEnv

    ds = SyntheticShapeNet(n_models=8, seed=1234)
    environment.seed_scene_rng(78)
    np.random.seed(78)
    torch.manual_seed(78)
    venv = SimpleVecEnv([lambda: OcclusionEnv(ds, img_size=64) for _ in range(4)])
    enc = nets[("predictor", 1)][3]
    net = TrainableSeparableEncoder.from_encoder(enc)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    res = harness.train_predictor(venv, net, 4)
    assert res["net"] is net and res["steps"] + res["skipped"] == 4 and res["steps"] >= 1
    assert len(res["losses"]) == res["steps"] and all(np.isfinite(v) for v in res["losses"])
    assert all(not torch.equal(v, before[k]) for k, v in net.named_parameters())
    res = harness.train_predictor(venv, enc, 1)  # from a separable encoder: the separable net is made
    assert isinstance(res["net"], TrainableSeparableEncoder)
    res = harness.train_predictor(venv, nets[("golden", 2)][3], 1)  # the "ppo" preset, dilation 2, gradPredictor head
    assert isinstance(res["net"], TrainableSeparableEncoder) and res["net"].enc.dilation == 2
